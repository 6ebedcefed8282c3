"""
GPU tests of the staged device encode (include/mrc_hip.h: mrc_dev_mdct, mrc_dev_smr, mrc_dev_alloc_quant, and the plain
mrc_dev_encode wrapper) and of timing mode (mrc_set_timing, mrc_get_stage_ms, mrc_get_kernel_ms), through the C ABI with
torch tensors for device memory.

The stage calls reach code that the fused encode does not: smr_kernel without band peaks (MODE 0: in joint blocks all four
signals with no M/S switch, and thresholds for all four), band_stats_kernel for the per-band peaks the scale factors need,
and the M/S decision made inside the allocation stage.  Each stage is checked against the oracle (oracle.fast) with the
bars of test_gpu_parity.py -- every integer bit-exact, MDCT lines within 1e-12 of the peak, thresholds and SMRs within
1e-9 dB -- and the staged chain bit for bit against mrc_dev_encode_ex on the same inputs, in every frame layout, at frame
counts around the allocation's 64 frames per wave, on a stream other than the handle's.
"""
import numpy as np
import pytest

from oracle import fast
from test_gpu_shapes import _blocks, _pair

pytestmark = pytest.mark.gpu

MDCT_RTOL = 1e-12
DB_ATOL = 1e-9
SR = 48000
EXACT_SPREAD = 1                                             # MRC_OPT_EXACT_SPREAD
SENS = 5                                                     # MRC_OPT_SENSITIVITY
# the reference's four shapes, then shapes that reach other kernel instantiations (test_gpu_shapes.SHAPES)
SHAPES = [(1024, 1024), (128, 128), (1024, 128), (128, 1024),
          (576, 576), (96, 160), (144, 144), (162, 162), (486, 486), (896, 1152)]
N_NOISE = 8                                                  # noise blocks per case, before the edge blocks


@pytest.fixture(scope="module")
def h():
    from mrcaudiocodec_amd import Handle
    hd = Handle(device_id=0)
    yield hd
    hd.close()


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def _accepts(hd, a, b):
    from mrcaudiocodec_amd import MrcError
    try:
        hd.bands(a, b)
        return True
    except MrcError:
        return False


def _edges(a, b):
    """digital silence, a full-scale square wave, a tone 80 dB down (all on the 16-bit grid).  Neither sits on a bin of
    any block length here: a spectrum symmetric about a bin makes exact neighbour ties that the strict peak test
    (psychoac.py:162) decides by the last bit of the FFT -- the near-ties test_gpu_sensitivity.py crafts on purpose."""
    from mrcaudiocodec_amd import synth
    t = np.arange(a + b)
    square = np.where((t // 23) % 2 == 0, 32767, -32767)
    quiet = np.rint(32767 * 1e-4 * np.sin(2 * np.pi * 997.0 / SR * t))
    return synth.pcm_to_float(np.stack([np.zeros(a + b), square, quiet]))


def _inputs(a, b, joint, seed):
    """mono: noise + tone blocks and the edge blocks; joint: correlated and independent pairs, edge pairs, and L == R
    (S is silent, the two streams tie)"""
    e = _edges(a, b)
    if not joint:
        return np.vstack([_blocks(a, b, N_NOISE, seed), e]), None
    left, right = _pair(a, b, N_NOISE, seed)
    el = np.vstack([e, left[:1]])                            # silence | square | quiet | a noise block
    er = np.vstack([e[0], e[1], e[0], left[:1]])             # silence | the same square | silence | the same block
    return np.vstack([left, el]), np.vstack([right, er])


_REF = {}


def _ref(a, b, joint):
    """the oracle on the inputs of (a, b, joint): encodes with a varied reservoir and with none, every signal's thresholds"""
    key = (a, b, joint)
    if key not in _REF:
        left, right = _inputs(a, b, joint, seed=3 * a + b + joint)
        n = left.shape[0]
        res = np.random.default_rng(a + b).integers(1, 700, n)
        if joint:
            enc = lambda r: fast.encode_joint_batch(left, right, a, b, reservoir_in=r)
            sigs = [left, right, (left + right) / 2.0, (left - right) / 2.0]   # as encode_joint_batch forms them
        else:
            enc = lambda r: fast.encode_mono_batch(left, a, b, reservoir_in=r)
            sigs = [left]
        thr = np.stack([fast.masked_threshold_batch(s, (a + b) // 2, SR) for s in sigs], axis=1)
        _REF[key] = dict(left=left, right=right, res=res, zero=enc(None), varied=enc(res), thresh=thr)
    return _REF[key]


# ------------------------------------------------------------------ device buffers and the three stages
def _dev(torch, x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x).reshape(-1))
    return t.to(device="cuda:0", dtype=dtype or t.dtype)


def _full(torch, n, dtype, value):
    return torch.full((max(int(n), 1),), value, dtype=dtype, device="cuda:0")


def _ptr(t):
    return None if t is None else t.data_ptr()


class Stages:
    """the caller-owned buffers of one staged encode (filled with values no stage writes, so that an entry a kernel
    skipped shows up)"""

    def __init__(self, torch, hd, a, b, n, joint):
        self.torch, self.h, self.a, self.b, self.n, self.joint = torch, hd, a, b, n, joint
        self.half, self.nb = (a + b) // 2, len(hd.bands(a, b))
        self.nsig, self.ns = (4, 2) if joint else (1, 1)
        f64, i32 = torch.float64, torch.int32
        self.lines = _full(torch, n * self.nsig * self.half, f64, float("nan"))
        self.osc = _full(torch, n * self.nsig, i32, -77)
        self.smr = _full(torch, n * self.nsig * self.nb, f64, float("nan"))
        self.thresh = _full(torch, n * self.nsig * self.half, f64, float("nan"))
        self.sw = _full(torch, n * self.nb, i32, -1)
        self.ba = _full(torch, n * self.ns * self.nb, i32, -1)
        self.sf = _full(torch, n * self.ns * self.nb, i32, -1)
        self.mant = _full(torch, n * self.ns * self.half, i32, -1)
        self.ro = _full(torch, n, i32, -12345)

    def mdct(self, chl, chr, stride, offsets=None, stream=None):
        self.h.dev_mdct(self.a, self.b, self.n, _ptr(chl), _ptr(chr), stride, _ptr(offsets), _ptr(self.lines),
                        _ptr(self.osc), stream)

    def smr_stage(self, chl, chr, stride, offsets=None, want_thresh=True, stream=None):
        self.h.dev_smr(self.a, self.b, self.n, _ptr(chl), _ptr(chr), stride, _ptr(offsets), _ptr(self.lines), _ptr(self.osc),
                       _ptr(self.smr), _ptr(self.thresh) if want_thresh else None, stream)

    def alloc(self, res=None, lines=None, stream=None):
        self.h.dev_alloc_quant(self.a, self.b, self.n, self.joint, _ptr(self.lines if lines is None else lines), _ptr(self.osc),
                               _ptr(self.smr), _ptr(res), _ptr(self.sw) if self.joint else None, _ptr(self.ba),
                               _ptr(self.sf), _ptr(self.mant), _ptr(self.ro), stream)

    def chain(self, chl, chr, stride, offsets=None, res=None, stream=None):
        self.mdct(chl, chr, stride, offsets, stream)
        self.smr_stage(chl, chr, stride, offsets, True, stream)
        self.alloc(res, None, stream)

    def stage_out(self):
        n, s, half, nb = self.n, self.nsig, self.half, self.nb
        c = lambda t, k: t.cpu().numpy()[:k]
        return dict(lines=c(self.lines, n * s * half).reshape(n, s, half), overall_scale=c(self.osc, n * s).reshape(n, s),
                    smr=c(self.smr, n * s * nb).reshape(n, s, nb), thresh=c(self.thresh, n * s * half).reshape(n, s, half))

    def ints(self):
        n, ns, half, nb = self.n, self.ns, self.half, self.nb
        c = lambda t, k: t.cpu().numpy()[:k].astype(np.int64)
        out = dict(overall_scale=c(self.osc, n * self.nsig), bit_alloc=c(self.ba, n * ns * nb).reshape(n, ns, nb),
                   scale_factor=c(self.sf, n * ns * nb).reshape(n, ns, nb), mantissa=c(self.mant, n * ns * half).reshape(n, ns, half),
                   reservoir_out=c(self.ro, n))
        if self.joint:
            out["ms_switch"] = c(self.sw, n * nb).reshape(n, nb)
            out["overall_scale"] = out["overall_scale"].reshape(n, 4)
        else:
            for k in ("bit_alloc", "scale_factor", "mantissa"):
                out[k] = out[k][:, 0]
        return out


def _fused(torch, hd, a, b, n, chl, chr, stride, offsets=None, res=None, plain=False):
    """mrc_dev_encode_ex(F64, I32) -- or mrc_dev_encode with plain=True -- on the same inputs, into the layout of Stages"""
    o = Stages(torch, hd, a, b, n, chr is not None)
    if plain:
        hd.dev_encode(a, b, n, _ptr(chl), _ptr(chr), stride, _ptr(offsets), _ptr(res), _ptr(o.osc), _ptr(o.sw) if o.joint else None,
                      _ptr(o.ba), _ptr(o.sf), _ptr(o.mant), _ptr(o.ro), _ptr(o.lines))
    else:
        hd.dev_encode_ex(a, b, n, _ptr(chl), _ptr(chr), 0, stride, _ptr(offsets), _ptr(res), _ptr(o.osc),
                         _ptr(o.sw) if o.joint else None, _ptr(o.ba), _ptr(o.sf), _ptr(o.mant), 0, _ptr(o.ro), _ptr(o.lines))
    torch.cuda.synchronize()
    return o


def _int_keys(joint):
    return ("overall_scale", "bit_alloc", "scale_factor", "mantissa", "reservoir_out") + (("ms_switch",) if joint else ())


def _assert_ints(got, ref, joint, what):
    for k in _int_keys(joint):
        g, r = np.asarray(got[k]), np.asarray(ref[k]).astype(np.int64)
        assert g.shape == r.shape, (what, k, g.shape, r.shape)
        bad = np.argwhere(g != r)
        assert bad.size == 0, "%s %s: %d mismatching entries, first at %s" % (what, k, len(bad), bad[0])


def _assert_same(x, y, joint, what, lines=True):
    _assert_ints(x.ints(), y.ints(), joint, what)
    if lines:
        assert np.array_equal(x.stage_out()["lines"], y.stage_out()["lines"]), what + " lines"


def _case(torch, hd, a, b, joint):
    r = _ref(a, b, joint)
    n = r["left"].shape[0]
    chl, chr = _dev(torch, r["left"]), (_dev(torch, r["right"]) if joint else None)
    return r, n, chl, chr


def _check_stage_outputs(got, r, a, b, joint, what):
    ref = r["zero"]
    nsig = 4 if joint else 1
    n, half = r["left"].shape[0], (a + b) // 2
    X = np.asarray(ref["mdct"]).reshape(n, nsig, half)
    err = np.abs(got["lines"] - X).max()
    assert err <= MDCT_RTOL * np.abs(X).max(), "%s: MDCT error %g" % (what, err)
    assert np.array_equal(got["overall_scale"], np.asarray(ref["overall_scale"]).reshape(n, nsig)), what + " overall_scale"
    smr = np.asarray(ref["smr"]).reshape(n, nsig, -1)
    assert np.isfinite(got["smr"]).all() and np.abs(got["smr"] - smr).max() <= DB_ATOL, \
        "%s: SMR error %g dB" % (what, np.abs(got["smr"] - smr).max())
    assert np.isfinite(got["thresh"]).all() and np.abs(got["thresh"] - r["thresh"]).max() <= DB_ATOL, \
        "%s: threshold error %g dB" % (what, np.abs(got["thresh"] - r["thresh"]).max())


# ------------------------------------------------------------------ 1. each stage alone against the oracle
@pytest.mark.parametrize("joint", [False, True], ids=["mono", "joint"])
@pytest.mark.parametrize("ab", SHAPES)
def test_mdct_and_smr_stages_against_the_oracle(h, torch, ab, joint):
    a, b = ab
    if not _accepts(h, a, b):
        pytest.skip("the handle refuses (%d,%d)" % ab)
    r, n, chl, chr = _case(torch, h, a, b, joint)
    st = Stages(torch, h, a, b, n, joint)
    st.mdct(chl, chr, a + b)
    st.smr_stage(chl, chr, a + b)
    torch.cuda.synchronize()
    got = st.stage_out()
    _check_stage_outputs(got, r, a, b, joint, "%s joint=%d" % (ab, joint))
    # without thresholds: the same SMRs
    st.smr.fill_(float("nan"))
    st.smr_stage(chl, chr, a + b, want_thresh=False)
    torch.cuda.synchronize()
    assert np.abs(st.stage_out()["smr"] - got["smr"]).max() <= DB_ATOL


@pytest.mark.parametrize("joint", [False, True], ids=["mono", "joint"])
@pytest.mark.parametrize("ab", [(1024, 1024), (128, 128)])
def test_smr_stage_in_both_spreading_modes(h, torch, ab, joint):
    a, b = ab
    r, n, chl, chr = _case(torch, h, a, b, joint)
    try:
        for exact in (1, 0):
            h.set_option(EXACT_SPREAD, exact)
            st = Stages(torch, h, a, b, n, joint)
            st.mdct(chl, chr, a + b)
            st.smr_stage(chl, chr, a + b)
            torch.cuda.synchronize()
            _check_stage_outputs(st.stage_out(), r, a, b, joint, "%s joint=%d exact=%d" % (ab, joint, exact))
    finally:
        h.set_option(EXACT_SPREAD, 0)


# ------------------------------------------------------------------ 2. the allocation stage against the oracle's integers
@pytest.mark.parametrize("joint", [False, True], ids=["mono", "joint"])
@pytest.mark.parametrize("ab", SHAPES)
def test_alloc_quant_stage_against_the_oracle(h, torch, ab, joint):
    a, b = ab
    if not _accepts(h, a, b):
        pytest.skip("the handle refuses (%d,%d)" % ab)
    r, n, chl, chr = _case(torch, h, a, b, joint)
    what = "%s joint=%d" % (ab, joint)
    st = Stages(torch, h, a, b, n, joint)
    st.chain(chl, chr, a + b, res=_dev(torch, r["res"], torch.int32))
    torch.cuda.synchronize()
    _assert_ints(st.ints(), r["varied"], joint, what + " reservoir_in varied")
    st0 = Stages(torch, h, a, b, n, joint)
    st0.chain(chl, chr, a + b, res=None)                     # NULL reservoir_in: zeros
    torch.cuda.synchronize()
    _assert_ints(st0.ints(), r["zero"], joint, what + " reservoir_in NULL")
    # the lines at an 8-byte offset (quantize_kernel<..., -1> on the long block): the same integers
    buf = _full(torch, n * st0.nsig * st0.half + 2, torch.float64, float("nan"))
    assert buf.data_ptr() % 16 == 0
    shifted = buf[1:1 + n * st0.nsig * st0.half]
    shifted.copy_(st0.lines[:shifted.numel()])
    torch.cuda.synchronize()
    st0.ba.fill_(-1); st0.sf.fill_(-1); st0.mant.fill_(-1); st0.sw.fill_(-1); st0.ro.fill_(-12345)
    st0.alloc(None, shifted)
    torch.cuda.synchronize()
    _assert_ints(st0.ints(), r["zero"], joint, what + " lines at an 8-byte offset")


# ------------------------------------------------------------------ 3. the staged chain equals the fused call
@pytest.mark.parametrize("joint", [False, True], ids=["mono", "joint"])
@pytest.mark.parametrize("ab", SHAPES)
def test_staged_chain_equals_fused_encode(h, torch, ab, joint):
    a, b = ab
    if not _accepts(h, a, b):
        pytest.skip("the handle refuses (%d,%d)" % ab)
    r, n, chl, chr = _case(torch, h, a, b, joint)
    what = "%s joint=%d" % (ab, joint)
    res = _dev(torch, r["res"], torch.int32)
    st = Stages(torch, h, a, b, n, joint)
    st.chain(chl, chr, a + b, res=res)
    torch.cuda.synchronize()
    ex = _fused(torch, h, a, b, n, chl, chr, a + b, res=res)
    _assert_same(st, ex, joint, what + " staged vs dev_encode_ex")
    plain = _fused(torch, h, a, b, n, chl, chr, a + b, res=res, plain=True)
    _assert_same(plain, ex, joint, what + " dev_encode vs dev_encode_ex")


# ------------------------------------------------------------------ 4. layouts and frame counts
def _stream_case(a, b, n, joint, seed):
    """a stream read hop-overlapped (frame f at f*b), and explicit odd, non-monotone offsets into the same stream"""
    from mrcaudiocodec_amd import synth
    N = a + b
    length = (n - 1) * b + N + 7
    rng = np.random.default_rng(seed)
    level = np.repeat(rng.choice([100.0, 1000.0, 4000.0, 12000.0], size=length // 256 + 1), 256)[:length]
    px = np.clip(np.rint(rng.normal(0, 1, length) * level + 1500 * np.sin(np.arange(length) * 0.131)), -32767, 32767)
    x = synth.pcm_to_float(px)
    y = synth.pcm_to_float(np.clip(np.rint(0.8 * px + rng.normal(0, 400, length)), -32767, 32767)) if joint else None
    offs = rng.integers(0, length - N, n)                    # (every block inside the stream: offs | 1 <= length - N)
    offs[::2] |= 1                                           # odd sample offsets ...
    offs[0] = length - N                                     # ... out of order
    if n > 1:
        offs[1] = 1
    return x, y, offs.astype(np.int64)


def _stacked(x, starts, N):
    return np.stack([x[s:s + N] for s in starts])


@pytest.mark.parametrize("joint", [False, True], ids=["mono", "joint"])
@pytest.mark.parametrize("ab,n", [((1024, 1024), 1), ((1024, 1024), 63), ((1024, 1024), 64), ((1024, 1024), 65),
                                  ((1024, 1024), 300), ((128, 128), 1), ((128, 128), 65), ((144, 144), 300),
                                  ((1024, 128), 65)])
def test_staged_chain_layouts_and_counts(h, torch, ab, n, joint):
    a, b = ab
    N = a + b
    x, y, offs = _stream_case(a, b, n, joint, seed=n + a)
    assert len(np.unique(np.diff(offs))) > 1 or n < 3
    sx, sy = _dev(torch, x), (_dev(torch, y) if joint else None)
    hop = np.arange(n) * b
    ref = {}
    for name, starts in (("stream", hop), ("offsets", offs)):
        bl, br = _dev(torch, _stacked(x, starts, N)), (_dev(torch, _stacked(y, starts, N)) if joint else None)
        st = Stages(torch, h, a, b, n, joint)
        st.chain(bl, br, N)
        torch.cuda.synchronize()
        ref[name] = st
        # the fused call on the stacked blocks: the same integers (band peaks and M/S switch from another kernel)
        _assert_same(st, _fused(torch, h, a, b, n, bl, br, N), joint, "%s n=%d %s stacked vs fused" % (ab, n, name))
    lay = Stages(torch, h, a, b, n, joint)
    lay.chain(sx, sy, b)                                     # frame_stride = b: the hop-overlapped stream
    torch.cuda.synchronize()
    _assert_same(lay, ref["stream"], joint, "%s n=%d hop layout" % (ab, n), lines=ab == (1024, 1024))
    lay = Stages(torch, h, a, b, n, joint)
    lay.chain(sx, sy, N, offsets=_dev(torch, offs))
    torch.cuda.synchronize()
    _assert_same(lay, ref["offsets"], joint, "%s n=%d offsets" % (ab, n), lines=ab == (1024, 1024))


# ------------------------------------------------------------------ 5. the caller's stream
@pytest.mark.parametrize("joint", [False, True], ids=["mono", "joint"])
def test_stages_on_a_stream_of_the_callers(h, torch, joint):
    a, b = 1024, 1024
    r, n, chl, chr = _case(torch, h, a, b, joint)
    res = _dev(torch, r["res"], torch.int32)
    base = Stages(torch, h, a, b, n, joint)
    base.chain(chl, chr, a + b, res=res)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())            # (inputs and buffers were written on torch's stream)
    st = Stages(torch, h, a, b, n, joint)
    torch.cuda.synchronize()
    st.chain(chl, chr, a + b, res=res, stream=side.cuda_stream)
    side.synchronize()                                       # that stream only
    _assert_same(st, base, joint, "side stream")
    for k in ("smr", "thresh"):
        assert np.array_equal(st.stage_out()[k], base.stage_out()[k]), k
    _assert_ints(st.ints(), r["varied"], joint, "side stream vs oracle")


# ------------------------------------------------------------------ 6. edges
def test_stage_edges(h, torch):
    from mrcaudiocodec_amd import MrcError
    a, b = 1024, 1024
    ch = _full(torch, 2 * (a + b), torch.float64, 0.0)
    for joint in (False, True):
        st = Stages(torch, h, a, b, 1, joint)
        chr = ch if joint else None
        # no frames: nothing to do, and OK
        h.dev_mdct(a, b, 0, _ptr(ch), _ptr(chr), a + b, None, _ptr(st.lines), _ptr(st.osc))
        h.dev_smr(a, b, 0, _ptr(ch), _ptr(chr), a + b, None, _ptr(st.lines), _ptr(st.osc), _ptr(st.smr), _ptr(st.thresh))
        h.dev_alloc_quant(a, b, 0, joint, _ptr(st.lines), _ptr(st.osc), _ptr(st.smr), None, _ptr(st.sw), _ptr(st.ba),
                          _ptr(st.sf), _ptr(st.mant), _ptr(st.ro))
        torch.cuda.synchronize()
        assert (st.osc.cpu().numpy() == -77).all() and (st.ro.cpu().numpy() == -12345).all()
        bad = [
            lambda: h.dev_smr(a, b, 1, _ptr(ch), _ptr(chr), a + b, None, _ptr(st.lines), _ptr(st.osc), None, None),
            lambda: h.dev_alloc_quant(a, b, 1, joint, _ptr(st.lines), _ptr(st.osc), None, None, _ptr(st.sw), _ptr(st.ba),
                                      _ptr(st.sf), _ptr(st.mant), _ptr(st.ro)),
            lambda: h.dev_mdct(a, b, 1, _ptr(ch), _ptr(chr), a + b, None, None, _ptr(st.osc)),
            lambda: h.dev_smr(a, b, 1, _ptr(ch), _ptr(chr), a + b, None, None, _ptr(st.osc), _ptr(st.smr), None),
            lambda: h.dev_alloc_quant(a, b, 1, joint, None, _ptr(st.osc), _ptr(st.smr), None, _ptr(st.sw), _ptr(st.ba),
                                      _ptr(st.sf), _ptr(st.mant), _ptr(st.ro)),
            # a shape the handle refuses (test_gpu_shapes.REFUSED)
            lambda: h.dev_mdct(1152, 1152, 1, _ptr(ch), _ptr(chr), a + b, None, _ptr(st.lines), _ptr(st.osc)),
            lambda: h.dev_smr(1152, 1152, 1, _ptr(ch), _ptr(chr), a + b, None, _ptr(st.lines), _ptr(st.osc), _ptr(st.smr), None),
            lambda: h.dev_alloc_quant(1152, 1152, 1, joint, _ptr(st.lines), _ptr(st.osc), _ptr(st.smr), None, _ptr(st.sw),
                                      _ptr(st.ba), _ptr(st.sf), _ptr(st.mant), _ptr(st.ro)),
        ]
        if joint:                                            # joint without an M/S switch buffer
            bad.append(lambda: h.dev_alloc_quant(a, b, 1, True, _ptr(st.lines), _ptr(st.osc), _ptr(st.smr), None, None,
                                                 _ptr(st.ba), _ptr(st.sf), _ptr(st.mant), _ptr(st.ro)))
        for i, call in enumerate(bad):
            with pytest.raises(MrcError):
                call()
        torch.cuda.synchronize()
        assert (st.osc.cpu().numpy() == -77).all() and (st.ro.cpu().numpy() == -12345).all()


# ------------------------------------------------------------------ timing mode
def _check_times(hd, what):
    k, s = hd.kernel_ms(), hd.stage_ms()
    assert np.isfinite(k).all() and (k >= 0).all(), (what, k)
    assert k[0] > 0 and k[1] > 0, (what, k)                  # MDCT, smr_kernel
    assert np.array_equal(s, [k[0], k[1], k[2] + k[3] + k[4]]), (what, s, k)


def _same(x, y, what):
    assert x.keys() == y.keys(), what
    for k in x:
        if x[k] is not None:
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), (what, k)


@pytest.mark.parametrize("joint", [False, True], ids=["mono", "joint"])
def test_timing_mode_changes_no_output(h, torch, joint):
    a, b = 1024, 1024
    left, right = _pair(a, b, 80, seed=17)
    pcm = [np.clip(np.rint(np.random.default_rng(s).normal(0, 3000, 71 * 1024)), -32767, 32767).astype(np.int16)
           for s in (1, 2)]
    chl, chr = _dev(torch, left), (_dev(torch, right) if joint else None)

    def host(n):
        if joint:
            return h.encode_joint(left[:n], right[:n], a, b, want_mdct=True)
        return h.encode_mono(left[:n], a, b, want_mdct=True)

    def dev():
        o = _fused(torch, h, a, b, 80, chl, chr, a + b)
        return dict(o.ints(), lines=o.stage_out()["lines"])

    def stream():
        return h.encode_stream_pcm16(pcm[0], pcm[1] if joint else None, chunk_frames=16)

    calls = [("few blocks", lambda: host(12)), ("batch", lambda: host(80)), ("dev_encode_ex", dev),
             ("encode_stream_pcm16", stream)]
    h.set_timing(False)
    off = [f() for _, f in calls]
    h.set_timing(True)
    try:
        for (what, f), want in zip(calls, off):
            _same(f(), want, what)
            if what != "encode_stream_pcm16":                # (its pipeline overlaps calls: not timed)
                _check_times(h, what)
    finally:
        h.set_timing(False)


@pytest.mark.parametrize("joint", [False, True], ids=["mono", "joint"])
def test_stream_encode_leaves_timing_on(joint):
    from mrcaudiocodec_amd import Handle
    hd = Handle(device_id=0)                                 # (a fresh handle: no time of an earlier call to report)
    try:
        pcm = np.clip(np.rint(np.random.default_rng(5).normal(0, 3000, (2, 9 * 1024))), -32767, 32767).astype(np.int16)
        hd.set_timing(True)
        hd.encode_stream_pcm16(pcm[0], pcm[1] if joint else None, chunk_frames=3)
        hd.encode_mono(_blocks(1024, 1024, 4, seed=9), 1024, 1024)
        _check_times(hd, "encode_mono after encode_stream_pcm16")
    finally:
        hd.close()
