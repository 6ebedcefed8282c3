"""
smr_kernel's front end requests the raw words of all of a thread's sample pairs (and their Hann values) before it
converts the first, in one arm per (alignment, signal kind) chosen once per unit.  Which arm a unit takes depends on the
parity of the channel's base address and of the block's offset, and on the signal; none of that may change a result.

int16 PCM through StreamEncoder.encode / encode_long.  Every frame a case encodes starts at one of a fixed pool of
positions of ONE stream (frames are independent: no reservoir is carried), so the three references are computed once per
position and shared: the frame encoded alone, the float64-input path on the mapped samples, and the oracle.
"""
import numpy as np
import pytest

import mono_oracle
from oracle import fast

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

INT_KEYS = ("overall_scale", "scale_factor", "bit_alloc", "mantissa", "reservoir_out")
HOP = 1024
BIG = 259                     # frames of the largest batch (no warm-up distance is shipped: 67 and 259)
BATCHES = (1, 2, 9, 67, BIG)
NPOS = BIG + 1                # positions per parity: k * HOP and 1 + k * HOP, k < NPOS


def _noise(n, seed, sigma=0.1):
    return np.clip(np.rint(np.random.default_rng(seed).normal(0, sigma * 32767, n)), -32768, 32767).astype(np.int16)


def _with_extremes(p):
    """-32768 and +32767 in every hop: in the low and in the high half of an aligned word, and as both halves of one"""
    p = p.copy()
    for r, c in ((100, -32768), (357, -32768), (612, 32767), (869, 32767), (200, -32768), (201, -32768), (440, 32767),
                 (441, -32768)):
        p[r::HOP] = c
    return p


class _Kit:
    def __init__(self):
        from mrcaudiocodec_amd import Handle
        from mrcaudiocodec_amd.batch import StreamEncoder
        self.h = Handle(device_id=0)
        self.enc = StreamEncoder(self.h)
        self.dev = self.enc.device
        n = (NPOS + 2) * HOP + 2
        self.pcm = _with_extremes(_noise(n, 31))
        self.t16 = torch.from_numpy(self.pcm).to(self.dev)
        self.t64 = torch.from_numpy(mono_oracle.to_float(self.pcm)).to(self.dev)
        self._refs = None

    def run(self, a, b, left, right, n, stride, offsets=None):
        to = None if offsets is None else torch.from_numpy(np.asarray(offsets, dtype=np.int64)).to(self.dev)
        out = self.enc.encode(a, b, left, right, n, stride, to, fresh=True)
        torch.cuda.synchronize(self.dev)
        return {k: v.cpu().numpy() for k, v in out.items()}

    def refs(self):
        """per pool position (index 2 k + parity): the frame alone from int16, alone from float64, and the oracle's"""
        if self._refs is None:
            pos = np.array([k * HOP + par for k in range(NPOS) for par in (0, 1)], dtype=np.int64)
            alone = [self.run(HOP, HOP, self.t16, None, 1, 0, [p]) for p in pos]
            one = {k: np.concatenate([r[k] for r in alone]) for k in INT_KEYS}
            f64 = self.run(HOP, HOP, self.t64, None, len(pos), 0, pos)
            x = mono_oracle.to_float(self.pcm)
            blocks = np.stack([x[p:p + 2 * HOP] for p in pos])
            orc = fast.encode_mono_batch(blocks, HOP, HOP)
            self._refs = dict(one=one, f64={k: f64[k] for k in INT_KEYS}, oracle={k: np.asarray(orc[k]) for k in INT_KEYS})
        return self._refs


@pytest.fixture(scope="module")
def kit():
    k = _Kit()
    yield k
    k.h.close()


def _pool_index(absolute):
    absolute = np.asarray(absolute)
    return 2 * (absolute // HOP) + (absolute % HOP)


def _check(got, refs, idx, what):
    for name, ref in refs.items():
        for k in INT_KEYS:
            g = np.squeeze(got[k]).astype(np.int64)
            r = np.squeeze(ref[k][idx]).astype(np.int64)
            assert g.shape == r.shape, (what, name, k, g.shape, r.shape)
            assert np.array_equal(g, r), (what, name, k)


def test_references_agree_and_contain_the_extreme_codes(kit):
    r = kit.refs()
    assert (kit.pcm[:2 * HOP] == -32768).sum() >= 8 and (kit.pcm[:2 * HOP] == 32767).sum() >= 6
    for k in INT_KEYS:
        assert np.array_equal(np.squeeze(r["one"][k]).astype(np.int64), np.squeeze(r["oracle"][k]).astype(np.int64)), k
        assert np.array_equal(r["one"][k], r["f64"][k]), k


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("layout", ["streamed", "odd_offsets", "shuffled_offsets"])
@pytest.mark.parametrize("base", [0, 1])
def test_mono_long_batches(kit, base, layout, n):
    """base 1: the channel is a view that starts one sample in (its address is no multiple of the pair size)"""
    left = kit.t16[base:]
    if layout == "streamed":
        absolute = base + HOP * np.arange(n)
        got = kit.run(HOP, HOP, left, None, n, HOP)
    else:
        if layout == "odd_offsets":
            offsets = (1 if base == 0 else HOP - 1) + HOP * np.arange(n)
            assert (offsets % 2 == 1).all()
        else:
            rng = np.random.default_rng(1000 * base + n)
            absolute = rng.permutation(np.array([k * HOP + par for k in range(1, NPOS) for par in (0, 1)]))[:n]
            offsets = absolute - base
        absolute = base + offsets
        got = kit.run(HOP, HOP, left, None, n, 0, offsets)
    _check(got, kit.refs(), _pool_index(absolute), (base, layout, n))


def _joint_stream(n_hops):
    """C3-like int16 stereo in three kinds of hop runs: R = L (every band M/S: the L and R units have no reader and
    return early), an unrelated and much quieter R (every band L/R: the M and S units return early), and a partly
    correlated mix"""
    n = (n_hops + 2) * HOP + 2
    t = np.arange(n)
    tone = np.rint(3000 * np.sin(2 * np.pi * 440.0 / 48000 * t)).astype(np.int64)
    pl = _with_extremes(np.clip(_noise(n, 41, 0.05).astype(np.int64) + tone, -32768, 32767).astype(np.int16))
    other = _noise(n, 42, 0.2)
    pr = pl.copy()
    third = (n_hops // 3 + 1) * HOP
    # (ms_stereo.py:5-27 codes a band as L / R when |l^2 - r^2| >= 0.8 (l^2 + r^2): an unrelated channel 22 dB down)
    pr[third:2 * third] = _noise(n, 43, 0.004)[third:2 * third]
    mix = 0.8 * pl[2 * third:].astype(np.float64) + 0.2 * other[2 * third:]
    pr[2 * third:] = np.clip(np.rint(mix), -32768, 32767).astype(np.int16)
    return pl, pr


@pytest.mark.parametrize("n", [3, 9])
@pytest.mark.parametrize("base", [0, 1])
def test_joint_long_batches(kit, base, n):
    pl, pr = _joint_stream(12)
    keys = INT_KEYS + ("ms_switch",)
    tl, tr = torch.from_numpy(pl).to(kit.dev)[base:], torch.from_numpy(pr).to(kit.dev)[base:]
    fl, fr = mono_oracle.to_float(pl), mono_oracle.to_float(pr)
    tl64, tr64 = torch.from_numpy(fl).to(kit.dev)[base:], torch.from_numpy(fr).to(kit.dev)[base:]
    first = {3: 0, 9: 2}[n]                                   # (nine frames: across all three kinds of run)
    for offsets in (None, (first + np.arange(n)) * HOP + 1, ((first + np.arange(n)) * HOP)[::-1].copy()):
        if offsets is None:
            got = kit.run(HOP, HOP, tl[first * HOP:], tr[first * HOP:], n, HOP)
            absolute = base + (first + np.arange(n)) * HOP
        else:
            got = kit.run(HOP, HOP, tl, tr, n, 0, offsets)
            absolute = base + offsets
        alone = [kit.run(HOP, HOP, tl, tr, 1, 0, [o - base]) for o in absolute]
        f64 = kit.run(HOP, HOP, tl64, tr64, n, 0, absolute - base)
        want = fast.encode_joint_batch(np.stack([fl[o:o + 2 * HOP] for o in absolute]),
                                       np.stack([fr[o:o + 2 * HOP] for o in absolute]), HOP, HOP)
        for k in keys:
            assert np.array_equal(got[k], np.concatenate([r[k] for r in alone])), (base, n, k, "alone")
            assert np.array_equal(got[k], f64[k]), (base, n, k, "float64")
            assert np.array_equal(np.squeeze(got[k]).astype(np.int64), np.squeeze(want[k]).astype(np.int64)), (base, n, k, "oracle")
        ms = got["ms_switch"] != 0
        if n == 9:
            assert ms.all(axis=1).any() and (~ms.any(axis=1)).any()       # frames whose L / R, and whose M / S units, return early
        else:
            assert ms.all(axis=1).all()                                    # R = L: every L and R unit returns early


@pytest.mark.parametrize("joint", [False, True])
@pytest.mark.parametrize("ab", [(1024, 128), (128, 128), (768, 768)])     # transition, short, generic kernel
def test_other_shapes(kit, ab, joint):
    a, b = ab
    keys = INT_KEYS + (("ms_switch",) if joint else ())
    pl, pr = _joint_stream(16)
    offsets = np.array([0, 1, 2048, 4097, 9000, 12345, 7, 1024, 5121, 3000, 15001, 6144, 11, 8192], dtype=np.int64)
    fl, fr = mono_oracle.to_float(pl), mono_oracle.to_float(pr)
    for base in (0, 1):
        tl = torch.from_numpy(pl).to(kit.dev)[base:]
        tr = torch.from_numpy(pr).to(kit.dev)[base:] if joint else None
        got = kit.run(a, b, tl, tr, len(offsets), 0, offsets)
        alone = [kit.run(a, b, tl, tr, 1, 0, [o]) for o in offsets]
        bl = np.stack([fl[base + o:base + o + a + b] for o in offsets])
        if joint:
            want = fast.encode_joint_batch(bl, np.stack([fr[base + o:base + o + a + b] for o in offsets]), a, b)
        else:
            want = fast.encode_mono_batch(bl, a, b)
        for k in keys:
            assert np.array_equal(got[k], np.concatenate([r[k] for r in alone])), (ab, joint, base, k, "alone")
            assert np.array_equal(np.squeeze(got[k]).astype(np.int64), np.squeeze(want[k]).astype(np.int64)), (ab, joint, base, k, "oracle")
