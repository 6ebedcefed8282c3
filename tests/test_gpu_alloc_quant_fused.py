"""
GPU tests of the long block's back end, alloc_quant_long_kernel (csrc/mrc_kernels_alloc.hip): bit allocation, scale factors
and mantissas of 64 frames per workgroup in one kernel.  It serves 1024 lines x 25 bands with 16-byte aligned planes; every
other shape and alignment keeps bitalloc_kernel + quantize_kernel.

Yardsticks: the oracle's integers (oracle.fast, as tests/test_gpu_parity.py obtains them), bit for bit; and, where noted,
the few-block path -- calls of <= 64 blocks through encode_mono / encode_joint take the event-list back end, which shares
no kernel with this one.  Every device call goes through mrc_dev_encode_ex or the stage entry mrc_dev_alloc_quant with torch
tensors for device memory; every output plane has one frame's worth of a fill value behind it that must survive.
"""
import numpy as np
import pytest

from oracle import fast
from test_gpu_shapes import _blocks, _pair
from test_gpu_stages import Stages, _assert_ints, _dev, _full, _int_keys, _ptr

pytestmark = pytest.mark.gpu

A = B = HALF = 1024
NB = 25
N_ALL = 200                                                  # frames of the shared inputs; a case takes the first n
COUNTS = [1, 63, 64, 65, 129, 200]                           # around the workgroup's 64 frames
CANARY = -31000                                              # fits the uint16 plane too; no output takes this value
_PARAM = dict(sample_rate="sampleRate", n_scale_bits="nScaleBits", n_mant_size_bits="nMantSizeBits")


@pytest.fixture(scope="module")
def h():
    from mrcaudiocodec_amd import Handle
    hd = Handle(device_id=0)
    yield hd
    hd.close()


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


# ------------------------------------------------------------------ inputs and references, computed once
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _inputs(joint):
    """mono: noise of varying level plus a tone.  Joint, frame i by i % 3: R = L (every band M/S, the L / R units of smr_kernel
    are skipped) | independent channels (every band L/R) | the C3 recipe of bench.py, whose blocks span an M/S hop and an L/R
    hop, so that M/S and L/R bands meet inside a frame"""
    def make():
        from mrcaudiocodec_amd import synth
        left = _blocks(A, B, N_ALL, seed=11)
        if not joint:
            return left, None
        # independent of L and 20 dB below it (at equal levels independent noise still takes M/S in the wide bands)
        other = synth.pcm_to_float(np.rint(0.1 * np.rint(left[:, ::-1] * 32767.5)))
        s = synth.c3_stereo(N_ALL)
        c3l, c3r = np.array(fast.blocks_from_stream(s[0], 1024)), np.array(fast.blocks_from_stream(s[1], 1024))
        kind = (np.arange(N_ALL) % 3)[:, None]
        return np.where(kind == 2, c3l, left), np.where(kind == 0, left, np.where(kind == 1, other, c3r))
    return _cached(("in", joint), make)


def _res_varied():
    return np.random.default_rng(2048).integers(-100, 600, N_ALL)


def _oracle(joint, n, res, params=None, left=None, right=None):
    if left is None:
        left, right = _inputs(joint)
    if joint:
        return fast.encode_joint_batch(left[:n], right[:n], A, B, None if res is None else res[:n], params=params)
    return fast.encode_mono_batch(left[:n], A, B, None if res is None else res[:n], params=params)


def _ref(joint):
    """the oracle on all N_ALL frames with a varied reservoir (frames are independent: a case compares its first n)"""
    return _cached(("ref", joint), lambda: _oracle(joint, N_ALL, _res_varied()))


def _alone(hd, joint):
    """every frame encoded ALONE through the few-block path (one block per call)"""
    def make():
        left, right = _inputs(joint)
        res = _res_varied()
        outs = []
        for i in range(N_ALL):
            if joint:
                outs.append(hd.encode_joint(left[i:i + 1], right[i:i + 1], A, B, res[i:i + 1]))
            else:
                outs.append(hd.encode_mono(left[i:i + 1], A, B, res[i:i + 1]))
        return {k: np.concatenate([np.asarray(o[k]) for o in outs]) for k in _int_keys(joint)}
    return _cached(("alone", joint), make)


def _cut(ref, n, joint):
    return {k: np.asarray(ref[k])[:n] for k in _int_keys(joint)}


# ------------------------------------------------------------------ output planes with canaries
class Planes:
    """the output planes of one mrc_dev_encode_ex call, each followed by one frame's worth of CANARY"""

    def __init__(self, torch, n, joint, fmt16, nb=NB):
        self.torch, self.n, self.joint, self.nb = torch, n, joint, nb
        ns, nsig = (2, 4) if joint else (1, 1)
        self.ns, self.nsig = ns, nsig
        one = dict(osc=nsig, sw=nb, ba=ns * nb, sf=ns * nb, mant=ns * HALF, ro=1)
        self.size = {k: n * v for k, v in one.items()}
        self.t = {k: _full(torch, self.size[k] + v, torch.int16 if (k == "mant" and fmt16) else torch.int32, CANARY)
                  for k, v in one.items()}
        self.fmt = 1 if fmt16 else 0

    def encode(self, hd, chl, chr, res=None):
        t = self.t
        hd.dev_encode_ex(A, B, self.n, _ptr(chl), _ptr(chr), 0, A + B, None, _ptr(res), _ptr(t["osc"]),
                         _ptr(t["sw"]) if self.joint else None, _ptr(t["ba"]), _ptr(t["sf"]), _ptr(t["mant"]), self.fmt,
                         _ptr(t["ro"]), None)
        self.torch.cuda.synchronize()
        return self

    def _host(self, k):
        a = self.t[k].cpu().numpy()
        if a.dtype == np.int16:
            a = a.view(np.uint16)
        return a.astype(np.int64)

    def ints(self):
        n, ns, nb = self.n, self.ns, self.nb
        c = lambda k: self._host(k)[:self.size[k]]
        out = dict(overall_scale=c("osc"), bit_alloc=c("ba").reshape(n, ns, nb), scale_factor=c("sf").reshape(n, ns, nb),
                   mantissa=c("mant").reshape(n, ns, HALF), reservoir_out=c("ro"))
        if self.joint:
            out["ms_switch"] = c("sw").reshape(n, nb)
            out["overall_scale"] = out["overall_scale"].reshape(n, 4)
        else:
            for k in ("bit_alloc", "scale_factor", "mantissa"):
                out[k] = out[k][:, 0]
        return out

    def assert_canaries(self, what):
        want = CANARY & 0xffff if self.fmt else CANARY
        for k in self.t:
            if k == "sw" and not self.joint:
                continue
            tail = self._host(k)[self.size[k]:]
            assert (tail == (want if k == "mant" else CANARY)).all(), "%s: %s written beyond frame n - 1" % (what, k)


def _channels(torch, joint, n, left=None, right=None):
    if left is None:
        left, right = _inputs(joint)
    return _dev(torch, left[:n]), (_dev(torch, right[:n]) if joint else None)


def _mixed_signal_groups(ref, n):
    """(frame, group of four lines) pairs whose lines lie in bands on BOTH sides of the M/S switch and have bits: the
    quantiser's oneSignal-false branch"""
    sfb = ref["sfBands"]
    band = np.repeat(np.arange(sfb.nBands), sfb.nLines)[:HALF].reshape(-1, 4)
    sw = np.asarray(ref["ms_switch"])[:n]
    bits = np.asarray(ref["bit_alloc"])[:n].reshape(n, 2, -1)
    split = sw[:, band[:, 0]] != sw[:, band[:, 3]]
    coded = (bits[:, 0][:, band[:, 0]] > 0) | (bits[:, 0][:, band[:, 3]] > 0)
    return int((split & coded).sum())


# ------------------------------------------------------------------ 1. frame counts at the workgroup edge
@pytest.mark.parametrize("fmt16", [False, True], ids=["i32", "u16"])
@pytest.mark.parametrize("joint", [False, True], ids=["mono", "joint"])
@pytest.mark.parametrize("n", COUNTS)
def test_frame_counts_at_the_workgroup_edge(h, torch, n, joint, fmt16):
    what = "n=%d joint=%d fmt16=%d" % (n, joint, fmt16)
    chl, chr = _channels(torch, joint, n)
    res = _dev(torch, _res_varied()[:n], torch.int32)
    p = Planes(torch, n, joint, fmt16).encode(h, chl, chr, res)
    got = p.ints()
    _assert_ints(got, _cut(_ref(joint), n, joint), joint, what + " vs oracle")
    _assert_ints(got, _cut(_alone(h, joint), n, joint), joint, what + " vs each frame alone, few-block path")
    p.assert_canaries(what)


# ------------------------------------------------------------------ 2. budgets: lanes of one wave leave the loop at different times
@pytest.mark.parametrize("joint", [False, True], ids=["mono", "joint"])
def test_budgets_mixed_in_one_batch(h, torch, joint):
    n = 130
    kind = np.arange(n) % 4
    # 0 | so negative that the budget is <= 0: no bits, all codes 0 | so large that every band retires at maxMantBits |
    # an ordinary reservoir
    res = np.choose(kind, [0, -1000000, 1000000, 300]).astype(np.int64)
    ref = _oracle(joint, n, res)
    ba = np.asarray(ref["bit_alloc"]).reshape(n, -1)
    assert (ba[kind == 1] == 0).all() and not np.asarray(ref["mantissa"])[kind == 1].any()
    assert (ba[kind == 2] == 16).all()
    assert len({tuple(r) for r in ba[kind == 0]}) > 1          # ordinary frames differ among themselves
    chl, chr = _channels(torch, joint, n)
    for fmt16 in (False, True):
        p = Planes(torch, n, joint, fmt16).encode(h, chl, chr, _dev(torch, res, torch.int32))
        _assert_ints(p.ints(), _cut(ref, n, joint), joint, "budgets joint=%d fmt16=%d" % (joint, fmt16))
        p.assert_canaries("budgets")


# ------------------------------------------------------------------ 3. joint selection
def test_joint_selection_three_kinds_of_frames(h, torch):
    n = 96
    ref = _ref(True)
    sw = np.asarray(ref["ms_switch"])[:n]
    kind = np.arange(n) % 3
    assert sw[kind == 0].all() and not sw[kind == 1].any()     # R = L: all M/S; independent channels: all L/R
    assert _mixed_signal_groups(ref, n) > 0                    # the C3 frames: four lines of one lane on two signals
    chl, chr = _channels(torch, True, n)
    res = _dev(torch, _res_varied()[:n], torch.int32)
    for fmt16 in (False, True):
        p = Planes(torch, n, True, fmt16).encode(h, chl, chr, res)
        _assert_ints(p.ints(), _cut(ref, n, True), True, "joint selection fmt16=%d" % fmt16)
        p.assert_canaries("joint selection")


def test_joint_unselected_signals_reach_no_decision(h, torch):
    """the stage entry, then again with NaN in what the switch does not select: the SMRs of every unselected (signal, band),
    and the M and S lines of L/R bands -- band_stats_kernel turns those into NaN band peaks.  (The L and R lines cannot be
    poisoned: the M/S decision itself reads them, ms_stereo.py:5-27.)"""
    n = 96
    chl, chr = _channels(torch, True, n)
    res = _dev(torch, _res_varied()[:n], torch.int32)
    st = Stages(torch, h, A, B, n, True)
    st.chain(chl, chr, A + B, res=res)
    torch.cuda.synchronize()
    want = st.ints()
    _assert_ints(want, _cut(_ref(True), n, True), True, "stage entry vs oracle")
    sw = want["ms_switch"].astype(bool)                        # [n][nb]
    selected = np.stack([~sw, ~sw, sw, sw], axis=1)            # [n][4][nb]: L, R, M, S
    smr = st.smr.cpu().numpy().reshape(n, 4, NB).copy()
    smr[~selected] = np.nan
    band = np.repeat(np.arange(NB), np.asarray(h.bands(A, B)))[:HALF]
    lines = st.lines.cpu().numpy().reshape(n, 4, HALF).copy()
    dead = ~selected[:, :, band]                               # [n][4][HALF]
    dead[:, :2] = False
    lines[dead] = np.nan
    assert np.isnan(smr).sum() == 2 * n * NB and np.isnan(lines).any()
    st.smr.copy_(_dev(torch, smr))
    st.lines.copy_(_dev(torch, lines))
    for t, v in ((st.ba, -1), (st.sf, -1), (st.mant, -1), (st.sw, -1), (st.ro, -12345)):
        t.fill_(v)
    st.alloc(res)
    torch.cuda.synchronize()
    _assert_ints(st.ints(), want, True, "NaN in the unselected signals")


# ------------------------------------------------------------------ 4. codec settings
SETTINGS = [dict(n_scale_bits=1, n_mant_size_bits=3),        # (scale factor -1 of a band without bits stays inside its byte)
            dict(n_scale_bits=2, n_mant_size_bits=8),
            dict(n_scale_bits=3, n_mant_size_bits=5, sample_rate=44100),
            dict(n_mant_size_bits=1)]


@pytest.mark.parametrize("joint", [False, True], ids=["mono", "joint"])
@pytest.mark.parametrize("kw", SETTINGS, ids=lambda kw: "-".join("%s=%s" % kv for kv in kw.items()))
def test_codec_settings(torch, kw, joint):
    from mrcaudiocodec_amd import Handle
    n = 70
    params = {_PARAM[k]: v for k, v in kw.items()}
    res = _res_varied()[:n]
    ref = _oracle(joint, n, res, params=params)
    hd = Handle(device_id=0, **kw)
    try:
        assert len(hd.bands(A, B)) == NB                       # the fused kernel's band count
        chl, chr = _channels(torch, joint, n)
        for fmt16 in (False, True):
            p = Planes(torch, n, joint, fmt16).encode(hd, chl, chr, _dev(torch, res, torch.int32))
            _assert_ints(p.ints(), _cut(ref, n, joint), joint, "%s joint=%d fmt16=%d" % (kw, joint, fmt16))
            p.assert_canaries(str(kw))
    finally:
        hd.close()


# ------------------------------------------------------------------ 5. the shapes that keep the two kernels
@pytest.mark.parametrize("joint", [False, True], ids=["mono", "joint"])
@pytest.mark.parametrize("which", ["lines", "mantissa"])
def test_fallback_planes_offset_by_8_bytes(h, torch, which, joint):
    n = 70
    chl, chr = _channels(torch, joint, n)
    res = _dev(torch, _res_varied()[:n], torch.int32)
    st = Stages(torch, h, A, B, n, joint)
    st.chain(chl, chr, A + B, res=res)
    torch.cuda.synchronize()
    want = _cut(_ref(joint), n, joint)
    _assert_ints(st.ints(), want, joint, "aligned")
    for t, v in ((st.ba, -1), (st.sf, -1), (st.mant, -1), (st.ro, -12345)):
        t.fill_(v)
    if which == "lines":
        buf = _full(torch, st.lines.numel() + 2, torch.float64, float("nan"))
        shifted = buf[1:1 + st.lines.numel()]
        shifted.copy_(st.lines)
        assert shifted.data_ptr() % 16 == 8
        st.alloc(res, shifted)
    else:
        buf = _full(torch, st.mant.numel() + 2 + st.ns * HALF, torch.int32, CANARY)
        st.mant = buf[2:]
        assert st.mant.data_ptr() % 16 == 8
        st.alloc(res)
    torch.cuda.synchronize()
    _assert_ints(st.ints(), want, joint, "%s at an 8-byte offset" % which)
    if which == "mantissa":
        assert (buf[:2].cpu().numpy() == CANARY).all() and (buf[2 + n * st.ns * HALF:].cpu().numpy() == CANARY).all()


@pytest.mark.parametrize("joint", [False, True], ids=["mono", "joint"])
def test_another_sample_rate_96k(torch, joint):
    """96 kHz: other band edges (bands of two lines at the bottom: a lane's four lines span up to three bands), a quiet
    threshold of +inf at the top.  The long block has 25 bands at every sample rate the codec accepts, so this handle takes the
    fused kernel too; a 1024-line block with another band count does not exist, the launcher's test of it is a guard."""
    from mrcaudiocodec_amd import Handle
    n = 70
    res = _res_varied()[:n]
    ref = _oracle(joint, n, res, params=dict(sampleRate=96000))
    hd = Handle(device_id=0, sample_rate=96000)
    try:
        nb = len(hd.bands(A, B))
        assert nb == ref["sfBands"].nBands and list(hd.bands(A, B)) != list(fast.bands_for(A, B).nLines)
        chl, chr = _channels(torch, joint, n)
        for fmt16 in (False, True):
            p = Planes(torch, n, joint, fmt16, nb=nb).encode(hd, chl, chr, _dev(torch, res, torch.int32))
            _assert_ints(p.ints(), _cut(ref, n, joint), joint, "96 kHz joint=%d fmt16=%d" % (joint, fmt16))
            p.assert_canaries("96 kHz")
    finally:
        hd.close()


# ------------------------------------------------------------------ 6. timing mode
@pytest.mark.parametrize("joint,n", [(False, 130), (True, 70)], ids=["mono-130", "joint-70"])
def test_timing_mode(h, torch, joint, n):
    chl, chr = _channels(torch, joint, n)
    res = _dev(torch, _res_varied()[:n], torch.int32)
    h.set_timing(False)
    want = Planes(torch, n, joint, True).encode(h, chl, chr, res).ints()
    h.set_timing(True)
    try:
        p = Planes(torch, n, joint, True).encode(h, chl, chr, res)
        k, s = h.kernel_ms(), h.stage_ms()
    finally:
        h.set_timing(False)
    assert np.isfinite(k).all() and (k >= 0).all(), k
    assert k[4] > 0, k                                         # the fused kernel, in the quantiser's slot
    assert s[2] == k[2] + k[3] + k[4], (s, k)
    _assert_ints(p.ints(), want, joint, "timed vs untimed")
    _assert_ints(want, _cut(_ref(joint), n, joint), joint, "untimed vs oracle")
    p.assert_canaries("timing")
