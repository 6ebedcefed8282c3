"""
GPU tests of smr_kernel (csrc/mrc_smr_body.hpp) around the second round of its masker table and under the cheap bounds of its
band contenders.  The table is built an entry per thread, 256 a round: a long block with more than 256 maskers has a second
round, run by wave 0 alone.  The mono long-block kernel then bounds every line's ratio -- since this test was written from the
`2^(j/256)` table alone, the hardware reciprocal and the high parts of the in-band prefix sums -- and evaluates only the lines
that can still be their band's maximum.  Neither the round a masker was made in nor the looseness of a bound may show anywhere.

The frames (tests/smr_overflow_inputs.py; what each reaches is asserted on the CPU by tests/test_smr_overflow_cpu.py): the
benchmark's noise with 255, 256, 257, 258 and 273 maskers, combs with more than 320, the step (contenders that fail the node
bound: chunks sent back), silence, impulse pairs (one of a single bit: table entries on the SPL floor) and a soft tone -- mono,
and as the L, R, M, S units of joint frames (a "mix" right channel), where the same counts come up in the joint instantiation.

Held, for batches of 1, 2 and 9 frames, hop-overlapped and by shuffled offsets[], from int16 and float64 samples:
  * every integer of an encode equals the oracle's (the harness of tests/test_gpu_smr_contenders.py);
  * the SMRs the encoder uses are within the project's 1e-9 dB of the oracle's;
  * smr_kernel's own outputs (SMRs and band peaks, through Handle.dev_masking) of a batch are bit for bit those of its frames
    taken one at a time, and the same from either sample format;
  * against tests/golden/smr_overflow_parent.npz -- the same outputs from the kernels of the commit before the cheap bounds,
    recorded on the GPU by tools/record_smr_overflow.py ("Cheap bounds for the band contenders") -- the band
    peaks are bit-equal and the SMRs within 1e-11 dB.  (Safe bounds change no bit: measured 0 dB.  The bound leaves room for
    arithmetic of a table entry that is worth a few 1e-13 dB -- the intensity formed without the level's round trip was tried
    with 2e-14 dB -- two orders below it, and stays two orders under the 1e-9 dB parity bar.);
  * with MRC_OPT_SENSITIVITY counting, no frame sends a chunk back from the nodes that the parent's kernel did not send.
"""
import os

import numpy as np
import pytest

from oracle import fast
import smr_overflow_inputs as I

HOP = I.HOP
COUNTS = (1, 2, 9)
DB_ATOL = 1e-9                                         # the project's bound (tests/test_gpu_parity.py)
PARENT_ATOL = 1e-11
INT_KEYS = ("overall_scale", "ms_switch", "bit_alloc", "scale_factor", "mantissa", "reservoir_out")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smr_overflow_parent.npz")

_cache = {}


@pytest.fixture(scope="module")
def dev():
    torch = pytest.importorskip("torch")
    from mrcaudiocodec_amd import Handle
    h = Handle(device_id=0)
    yield I.Device(torch, h)
    h.close()


def _ref(joint):
    """the oracle's encode of every frame, a row per label of I.all_labels(); computed once"""
    if ("ref", joint) not in _cache:
        left, right = I.blocks(I.all_labels())
        _cache["ref", joint] = fast.encode_joint_batch(left, right, HOP, HOP) if joint else fast.encode_mono_batch(left, HOP, HOP)
    return _cache["ref", joint]


def _singles(dev, joint, dtype="int16"):
    if ("one", joint, dtype) not in _cache:
        _cache["one", joint, dtype] = dev.singles(joint, dtype, I.all_labels())
    return _cache["one", joint, dtype]


def _used(joint, sw):
    """[n][nsig][nb]: the (signal, band) pairs whose SMR and peak the encoder takes (ms_stereo.py:70-81)"""
    if not joint:
        return np.ones((len(sw), 1, sw.shape[1]), dtype=bool)
    on = np.asarray(sw) != 0
    return np.stack([~on, ~on, on, on], axis=1)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


def _batches(n):
    """-> [(kind, row indices into I.all_labels(), masking() arguments)] of the batches of n frames"""
    labs, frames = I.all_labels(), I.stream()[1]
    last = [labs.index(lab) for lab in I.streamed_labels()[-n:]]
    pick = np.random.default_rng(n).permutation(len(I.labels()))[:n]
    if n == 2:
        pick = np.array([labs.index("c2-205"), labs.index("c2-13")])     # a second round next to none
    return [("streamed", last, dict(first=frames[labs[last[0]]], stride=HOP)),
            ("offsets", list(pick), dict(offsets=[frames[labs[i]] for i in pick]))]


@pytest.mark.gpu
@pytest.mark.parametrize("joint", [False, True], ids=["mono", "joint"])
def test_single_frames_against_the_oracle_and_the_parent(dev, joint):
    labs = I.all_labels()
    one, ref = _singles(dev, joint), _ref(joint)
    sw = ref["ms_switch"] if joint else np.zeros((len(labs), dev.nb), dtype=np.int64)
    if joint:
        assert np.array_equal(one["ms_switch"], sw)
    used = _used(joint, sw)
    want = ref["smr"].reshape(len(labs), -1, dev.nb)
    err = np.abs(one["smr"] - want)[used]
    print("largest |SMR - oracle| over %d values: %.3g dB" % (used.sum(), err.max()))
    assert not np.isnan(one["smr"][used]).any() and not np.isnan(one["band_peak"][used]).any()
    assert err.max() <= DB_ATOL
    # the other sample format: the same bits
    f64 = _singles(dev, joint, "float64")
    for k in one:
        assert _same_bits(one[k].astype(np.float64), f64[k].astype(np.float64)), k
    # the parent's kernels
    g = np.load(GOLDEN)
    assert list(g["labels"]) == labs
    tag = "joint" if joint else "mono"
    assert _same_bits(one["band_peak"], g["band_peak_" + tag]), "band peaks differ from the parent's"
    unwritten = np.isnan(g["smr_" + tag])
    assert np.array_equal(np.isnan(one["smr"]), unwritten)
    d = np.abs(one["smr"] - g["smr_" + tag])[~unwritten]
    print("largest |SMR - parent's| over %d values: %.3g dB" % (d.size, d.max()))
    assert d.max() <= PARENT_ATOL


@pytest.mark.gpu
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("dtype", ["int16", "float64"])
@pytest.mark.parametrize("joint", [False, True], ids=["mono", "joint"])
def test_batches_equal_single_frames(dev, joint, dtype, n):
    one = _singles(dev, joint)
    for kind, rows, args in _batches(n):
        got = dev.masking(joint, dtype, n, **args)
        for k in got:
            assert _same_bits(got[k].astype(np.float64), one[k][rows].astype(np.float64)), (kind, n, k)


@pytest.mark.gpu
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("joint", [False, True], ids=["mono", "joint"])
def test_encodes_equal_the_oracle(dev, joint, n):
    torch = dev.torch
    from mrcaudiocodec_amd.batch import StreamEncoder
    enc = StreamEncoder(handle=dev.h)
    ref = _ref(joint)
    for dtype in ("int16", "float64"):
        ch = dev.pcm[dtype]
        for kind, rows, args in _batches(n):
            first = args.get("first", 0)
            left = ch[0, first:].contiguous()
            right = ch[1, first:].contiguous() if joint else None
            off = torch.tensor(np.asarray(args["offsets"], dtype=np.int64), device="cuda:0") if "offsets" in args else None
            out = enc.encode(HOP, HOP, left, right, n, args.get("stride", 0), off, fresh=True)
            torch.cuda.synchronize()
            for k in INT_KEYS:
                if k in out:
                    got = np.squeeze(out[k].cpu().numpy()).astype(np.int64)
                    assert np.array_equal(got, np.squeeze(np.asarray(ref[k])[rows]).astype(np.int64)), (dtype, kind, n, k)


@pytest.mark.gpu
def test_no_frame_sends_back_a_chunk_the_parent_did_not_send(dev):
    labs = I.all_labels()
    got = dev.sent_back(labs)
    want = np.load(GOLDEN)["sent_back_mono"]
    print(dict(zip(labs, zip(got.tolist(), want.tolist()))))
    assert np.all(got <= want), "chunks sent back from the nodes (this kernel, the parent's)"
    assert all(got[labs.index(lab)] == 0 for lab in labs if lab.startswith("c2-")), "the benchmark's frames send none back"
    assert got[labs.index("step-4")] >= 1
