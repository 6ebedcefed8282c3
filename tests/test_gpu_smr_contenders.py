"""
GPU tests of the mono long-block smr_kernel's band contenders (csrc/mrc_smr_body.hpp): the kernel bounds every line's
ratio cheaply and evaluates the masked threshold in full only for the lines that can still be their band's maximum.  Which
lines those are must not show in any output: batches of 1, 2 and 9 frames of int16 PCM, read as a hop-overlapped stream and
through shuffled offsets[], are bit-identical to the same frames encoded one at a time, and every integer is the oracle's.

What each content exercises is ASSERTED on the CPU from the NumPy restatement of the selection rule
(tests/smr_contenders_restatement.py):

  noise     white noise of BASELINE config C2: ~257 maskers (both rounds of the node terms), every wave within capacity, every
            chunk through the gathered evaluation
  tone      997 Hz tone at half of full scale over a -60 dB noise floor: its slope range is too wide for the nodes, the frames
            take the sorted sweep (unchanged)
  softtone  the same tone at -36 dB: within the nodes' reach, contenders in the narrow bands, and a chunk with a line at the
            SPL floor guard (evaluated whole) in a frame that takes the nodes
  silence   hops of digital silence and of noise: blocks that are all silent (no masker), half silent and full -- and one
            half-silent block that puts MORE than the capacity into wave 0's lines (found by search on the CPU: that wave
            evaluates its four chunks whole)
  step      noise with a 40 dB step down at 6 kHz (sigma 0.1 of full scale; at 0.5 and 20 dB the slope range is beyond the
            nodes' reach): the node error bound fails for contenders above the step, whose chunks go back to the sorted sweep
  sparse    an impulse pair per block: 18 maskers, fewer than the 32 the nodes need (sorted sweep, unchanged)

That the send-back branch ran on the DEVICE is read from the sensitivity certificate (node chunks sent back: above zero for the
step, zero for noise, loud tone and sparse).

mrc_dev_smr launches the kernel without band peaks, i.e. not the mono instantiation: it never takes the contender path and
has no case here.
"""
import numpy as np
import pytest

from oracle import fast
import smr_contenders_restatement as R
from smr_content import content_noise, content_tone, content_softtone, content_silence, content_step, content_sparse

HOP = 1024
N_FRAMES = 9
COUNTS = (1, 2, 9)
INT_KEYS = ("overall_scale", "bit_alloc", "scale_factor", "mantissa", "reservoir_out")


CONTENTS = dict(noise=content_noise, tone=content_tone, softtone=content_softtone, silence=content_silence,
                step=content_step, sparse=content_sparse)


def blocks_of(pcm16):
    from mrcaudiocodec_amd import synth
    return np.array(fast.blocks_from_stream(synth.pcm_to_float(pcm16), HOP))


_cache = {}


def _corpus(name):
    """int16 codes of N_FRAMES + 1 hops, the oracle's encode of the N_FRAMES blocks and the restatement's account of each"""
    if name not in _cache:
        pcm = CONTENTS[name]()
        bl = blocks_of(pcm)
        assert bl.shape == (N_FRAMES, 2 * HOP)
        _cache[name] = dict(pcm=pcm, ref=fast.encode_mono_batch(bl, HOP, HOP), account=R.analyse_blocks(bl))
    return _cache[name]


def test_restatement_says_what_each_content_exercises():
    acc = {name: _corpus(name)["account"] for name in CONTENTS}
    nz = acc["noise"]
    assert all(a["nodes"] and not a["over_capacity"] and max(a["per_wave"]) <= R.CAPACITY for a in nz)
    assert all(a["contenders"] < 256 for a in nz), "fewer lines evaluated than a quarter of the frame"
    m = [a["maskers"] for a in nz[1:]]
    assert min(m) <= 256 < max(m) and 230 <= np.median(m) <= 290, m
    assert not any(a["whole_chunks"] for a in nz), "noise: every chunk through the gathered evaluation"
    # the loud tone: out of the nodes' reach although the masker count fits
    assert all(not a["nodes"] and R.NODE_MIN_MASKERS <= a["maskers"] <= R.NODE_MAX_MASKERS for a in acc["tone"])
    # the soft tone: nodes, contenders among wave 0's lines (chunk 0 holds the narrow bands), a floor chunk in the last frame
    assert all(a["nodes"] and a["per_wave"][0] >= 13 and not a["over_capacity"] for a in acc["softtone"])
    assert acc["softtone"][-1]["whole_chunks"] and not acc["softtone"][-1]["bound_fail_contenders"]
    # silence: all-silent blocks, half-silent ones that take the nodes, and the last frame over capacity in wave 0
    assert any(a["maskers"] == 0 for a in acc["silence"]) and any(a["nodes"] for a in acc["silence"])
    last = acc["silence"][-1]
    assert last["over_capacity"] and last["per_wave"][0] > R.CAPACITY and max(last["per_wave"][1:]) <= R.CAPACITY
    assert last["whole_chunks"] == set(R.wave_chunks(0))
    # the step: contenders whose error bound fails, in every frame (so in every batch)
    assert all(a["nodes"] and a["bound_fail_contenders"] >= 1 and a["whole_chunks"] for a in acc["step"])
    # sparse: outside the nodes' reach
    assert all(0 < a["maskers"] < R.NODE_MIN_MASKERS and not a["nodes"] for a in acc["sparse"])


@pytest.fixture(scope="module")
def h():
    from mrcaudiocodec_amd import Handle
    hd = Handle(device_id=0)
    yield hd
    hd.close()


def _encode(torch, enc, pcm, n, stride, offsets):
    lines = torch.full((n * HOP,), float("nan"), dtype=torch.float64, device="cuda:0")
    out = enc.encode(HOP, HOP, pcm, None, n, stride, offsets, lines_out=lines, fresh=True)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["lines"] = lines.cpu().numpy().reshape(n, 1, HOP)
    return res


_single = {}


def _one_at_a_time(torch, enc, name):
    if name not in _single:
        pcm = _corpus(name)["pcm"]
        rows = [_encode(torch, enc, torch.from_numpy(pcm[f * HOP:(f + 2) * HOP].copy()).to("cuda:0"), 1, HOP, None)
                for f in range(N_FRAMES)]
        _single[name] = {k: np.concatenate([r[k] for r in rows]) for k in rows[0]}
    return _single[name]


def _check_oracle(got, ref, idx):
    for k in INT_KEYS:
        want = np.asarray(ref[k])[idx]
        assert np.array_equal(np.squeeze(got[k]).astype(np.int64), np.squeeze(want).astype(np.int64)), k


@pytest.mark.gpu
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name", list(CONTENTS))
def test_batches_equal_single_frames_and_the_oracle(h, name, n):
    torch = pytest.importorskip("torch")
    from mrcaudiocodec_amd.batch import StreamEncoder
    enc = StreamEncoder(handle=h)
    c = _corpus(name)
    # a batch of n frames is the LAST n of the corpus (the first frame of some contents is half silent)
    first = N_FRAMES - n
    single = _one_at_a_time(torch, enc, name)
    dev = torch.from_numpy(c["pcm"][first * HOP:].copy()).to("cuda:0")
    assert dev.numel() == (n + 1) * HOP
    stream = _encode(torch, enc, dev, n, HOP, None)
    assert not np.isnan(stream["lines"]).any()
    for k in stream:
        assert np.array_equal(stream[k], single[k][first:]), (name, n, k)
    _check_oracle(stream, c["ref"], np.arange(first, N_FRAMES))
    order = np.random.default_rng(n).permutation(n)
    shuffled = _encode(torch, enc, dev, n, 0, torch.tensor(order.astype(np.int64) * HOP, device="cuda:0"))
    for k in shuffled:
        assert np.array_equal(shuffled[k], single[k][first + order]), (name, n, k)
    _check_oracle(shuffled, c["ref"], first + order)


@pytest.mark.gpu
def test_device_counts_the_chunks_contenders_send_back(h):
    """The restatement only approximates the kernel's arithmetic; that the send-back branch RAN is read from the device's own
    count (MRC_SENS_NODES): above zero for the step, whose contenders fail the bound in every frame by a wide margin, and zero
    where no contender fails it (noise) and where the frames do not take the nodes at all (loud tone, sparse)."""
    torch = pytest.importorskip("torch")
    from mrcaudiocodec_amd.batch import StreamEncoder
    enc = StreamEncoder(handle=h)
    assert all(a["bound_fail_contenders"] == 0 for name in ("noise", "tone", "sparse") for a in _corpus(name)["account"])
    h.set_option(5, 1)                                               # MRC_OPT_SENSITIVITY
    try:
        got = {}
        for name in ("noise", "tone", "sparse", "step"):
            h.sensitivity(reset=True)
            _encode(torch, enc, torch.from_numpy(_corpus(name)["pcm"].copy()).to("cuda:0"), N_FRAMES, HOP, None)
            got[name] = h.sensitivity(reset=True)
    finally:
        h.set_option(5, 0)
    print({k: v["node_chunks_sent_back"] for k, v in got.items()})
    assert all(v["blocks_examined"] == N_FRAMES for v in got.values()), got
    assert got["noise"]["node_chunks_sent_back"] == 0 and got["tone"]["node_chunks_sent_back"] == 0
    assert got["sparse"]["node_chunks_sent_back"] == 0
    # every frame of the step has chunks that its contenders send back (the restatement: 3 to 5 of them)
    assert got["step"]["node_chunks_sent_back"] >= N_FRAMES
