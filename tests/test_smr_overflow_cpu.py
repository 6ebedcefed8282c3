"""
CPU proof of what the frames of tests/test_gpu_smr_overflow.py (tests/smr_overflow_inputs.py) make the masker table of
smr_kernel do, from the NumPy account of the kernel's choices (tests/smr_paths_restatement.py, smr_contenders_restatement.py).

The table is built 256 maskers a round.  A long block with 256 or fewer has one round; with more, wave 0 runs a second one -- for
at most 64 maskers (257 .. 320) in every frame that can take the slope nodes, whose ceiling is 308.  The frames sit on either
side of both edges, in the mono and in the joint instantiation.

Run with -s to see the counts.
"""
import numpy as np

from oracle import fast
import smr_contenders_restatement as RC
import smr_overflow_inputs as I
import smr_paths_restatement as R

NT, WAVE = 256, 64                                     # table entries a round; a wave's worth of a second round
FLOOR_INTENSITY = 10.0 ** -12.6                        # an SPL reaches its -30 dB floor below it (psychoac.py:8-12)


def _acc():
    if "acc" not in I._cache:
        labs = I.all_labels()
        left, right = I.blocks(labs)
        sw, joint = R.joint_accounts(left, right, I.HOP, I.HOP)
        I._cache["acc"] = dict(labs=labs, mono={lab: R.account(b) for lab, b in zip(labs, left)},
                               joint={lab: row for lab, row in zip(labs, joint)},
                               contend={lab: a for lab, a in zip(labs, RC.analyse_blocks(left))}, left=left)
    return I._cache["acc"]


def test_the_benchmark_frames_sit_on_either_side_of_the_rounds_edge():
    from mrcaudiocodec_amd import synth
    a = _acc()
    assert {i: a["mono"]["c2-%d" % i]["maskers"] for i in I.C2_FRAMES} == I.C2_MASKERS
    assert sorted(I.C2_MASKERS.values())[:4] == [NT - 1, NT, NT + 1, NT + 2]
    assert all(a["mono"]["c2-%d" % i]["nodes"] for i in I.C2_FRAMES)
    assert all(a["contend"]["c2-%d" % i]["bound_fail_contenders"] == 0 for i in I.C2_FRAMES)
    # the stream the benchmark encodes: frames 1 .. 398 (frame 0 is half silent)
    x = synth.c2_noise(400)
    pcm, _ = I.stream()
    assert np.array_equal(synth.pcm_to_float(pcm[0, :I.C2_HOPS * I.HOP]), x[:I.C2_HOPS * I.HOP])
    m = np.array([R.maskers(x[f * I.HOP:f * I.HOP + I.N])["P"] for f in range(1, 399)])
    over = float((m > NT).mean())
    print("C2 frames 1..398: maskers %d..%d, median %d, %.0f %% above %d" % (m.min(), m.max(), np.median(m), 100 * over, NT))
    assert (m.min(), m.max(), int(np.median(m))) == (239, 273, 255) and 1 + int(m.argmax()) == 205
    assert 0.40 <= over <= 0.42 and m.max() <= NT + WAVE and m.max() <= R.CEILING[1024]
    # the streamed batches: second rounds and none, side by side
    s = [a["mono"][lab]["maskers"] for lab in I.streamed_labels()]
    assert any(v > NT for v in s) and any(v <= NT for v in s) and NT in s, s


def test_what_the_other_contents_reach():
    a = _acc()
    mono, con = a["mono"], a["contend"]
    print({lab: (v["maskers"], v["why"] or "nodes") for lab, v in mono.items()})
    # the combs: a second round of more than a wave's worth, more maskers than the nodes take
    assert mono["comb-4"]["maskers"] > NT + WAVE and mono["comb-4"]["why"] == "many"
    assert mono["comb-4"]["maskers"] >= 455                                            # (the scans' capacity: 461)
    assert mono["comb6-4"]["maskers"] > NT + WAVE and mono["comb6-4"]["why"] == "many"
    # the step: nodes, contenders that fail the bound, chunks sent back
    assert mono["step-4"]["nodes"] and mono["step-4"]["chunks"] and con["step-4"]["bound_fail_contenders"] >= 1
    # silence and the impulse pair: fewer than 32 maskers.  The silent frame's lines are on the SPL floor (4 xs^2 below the
    # floor's intensity); the impulse pair's are not (its quietest line is seven orders above it), whatever its name suggests
    assert mono["silence-1"]["maskers"] == 0 and mono["sparse-4"]["why"] == "few" and mono["sparse-4"]["maskers"] < 32
    labs = a["labs"]

    def quietest(lab):
        X = fast.mdct_batch(a["left"][labs.index(lab)][None, :], I.HOP, I.HOP)
        _, Xs = fast.overall_scale_batch(X, 4)
        return float((4.0 * Xs ** 2).min())
    assert quietest("silence-1") < FLOOR_INTENSITY < 1e-7 < quietest("sparse-4")
    # the pair of one least significant bit: every masker's level is the floor itself, its intensity 10^((-30 - 15 - 96) / 10)
    mk = R.maskers(a["left"][labs.index("lsb-0")])
    assert 0 < mk["P"] < 32 and np.all(mk["I"] == mk["I"][0]) and abs(mk["I"][0] / 10.0 ** -14.1 - 1) < 1e-12
    assert mono["lsb-0"]["why"] == "few"
    assert mono["silence-2"]["nodes"] and mono["silence-2"]["maskers"] < NT
    assert mono["softtone-4"]["nodes"] and con["softtone-4"]["contenders"] < 128


def test_joint_units_reach_every_kind_of_second_round():
    a = _acc()
    units = [(lab, s, acc) for lab in I.labels() for s, acc in enumerate(a["joint"][lab]) if acc["evaluated"]]
    counts = {lab: [acc["maskers"] for l2, _, acc in units if l2 == lab] for lab in I.labels()}
    print(counts)
    m = [acc["maskers"] for _, _, acc in units]
    second = [acc for _, _, acc in units if NT < acc["maskers"] <= NT + WAVE]
    assert len(second) >= 4 and all(acc["nodes"] or acc["why"] in ("slope", "many") for acc in second)
    assert any(acc["nodes"] for acc in second), "a second round in a unit through the nodes"
    assert any(v > NT + WAVE for v in m) and any(0 < v <= NT for v in m) and any(v == 0 for v in m)
    assert any(s >= 2 for _, s, _ in units) and any(s < 2 for _, s, _ in units)       # both sides of the M/S switch
