"""
GPU parity of the block shapes and codec settings the library accepts beyond the reference's four shapes at its default
settings -- through the C ABI, against the oracle (oracle.fast, oracle.decode, oracle.pacfile), with the bars of
test_gpu_parity.py: every integer bit-exact, MDCT lines within 1e-12 of the peak, the window within 4e-16, thresholds and
SMRs within 1e-9 dB; decoded blocks within 1e-12 of the peak (test_gpu_decode.py).

Each generic kernel instantiation (mdct_kernel, smr_kernel without a compile-time size, bitalloc_kernel<0>,
quantize_kernel<..., -1>) is reached only by such shapes or settings, and so is the choice between the few-block encode
(the chained back end, <= 64 blocks) and the batch path.  A shape the handle accepts (h.bands) must work at every entry
point; a shape whose kernels need more LDS than the device gives a workgroup is refused up front.
"""
import numpy as np
import pytest

from oracle import codec as ocodec, decode as odec, fast

pytestmark = pytest.mark.gpu

MDCT_RTOL = 1e-12
DB_ATOL = 1e-9
REF_SHAPES = [(1024, 1024), (128, 128), (1024, 128), (128, 1024)]

# (a, b): what the shape reaches
SHAPES = [
    (576, 576),      # N = 1152, not a transition: mdct_kernel (not mdct_wave_kernel); the transition-sized SMR kernel, other window
    (512, 640),      # N = 1152, shift +32: as above with an asymmetric window
    (640, 512),      # N = 1152, shift -32: as above, mirrored
    (96, 160),       # N = 256 with shift != 0: mdct_kernel<64>, the short-block SMR path with another window
    (160, 96),       # N = 256, mirrored
    (896, 1152),     # N = 2048, 25-band long table, asymmetric window: mdct_kernel<256>, long SMR, bitalloc_kernel<25>
    (108, 108),      # M <= 128 lines of no short size: smr_kernel<..., 128, 0, 0>
    (144, 144),      # generic 9-band shapes: smr_kernel<..., 0, 0>, quantize_kernel<..., -1>, bitalloc_kernel<0> (joint)
    (192, 192),
    (256, 256),
    (384, 384),
    (512, 512),
    (768, 768),
    (162, 162),      # halfN % 4 == 2: the few-block encode must not take the chained back end (it scans lines in fours)
    (160, 164),      # halfN % 4 == 2, asymmetric
    (486, 486),      # halfN % 4 == 2, 3-radix transforms
    # refused by the handle (h.bands): more peaks than smr_kernel's scan holds (N/2 > 1123), hence also more than 2048
    # coded lines per joint block (which the few-block encode and the chained encode would have to leave to other paths)
    (1152, 1152),
    (1536, 1536),
    (2048, 2048),    # ... and more LDS per workgroup
    (3072, 3072),    # more than 2048 lines even in mono
    (4096, 4096),    # also too many bands for the M/S summation plan
]
REFUSED = {(1152, 1152), (1536, 1536), (2048, 2048), (3072, 3072), (4096, 4096)}


@pytest.fixture(scope="module")
def h():
    from mrcaudiocodec_amd import Handle
    hd = Handle(device_id=0)
    yield hd
    hd.close()


def _accepts(hd, a, b):
    from mrcaudiocodec_amd import MrcError
    try:
        hd.bands(a, b)
        return True
    except MrcError:
        return False


def _blocks(a, b, n, seed):
    """n blocks of a+b samples on the 16-bit grid: noise whose level changes from block to block plus a tone"""
    from mrcaudiocodec_amd import synth
    rng = np.random.default_rng(seed)
    sigma = rng.choice([0.003, 0.03, 0.1, 0.4], size=n)[:, None]
    t = np.arange(a + b)[None, :] + np.arange(n)[:, None] * b
    x = rng.normal(0, 1, (n, a + b)) * sigma + 0.05 * np.sin(2 * np.pi * 1000.0 / 48000 * t)
    return synth.pcm_to_float(np.clip(np.rint(x * 32767), -32767, 32767))


def _pair(a, b, n, seed):
    """joint inputs: every other pair correlated (M/S bands), the others independent (L/R bands)"""
    left = _blocks(a, b, n, seed)
    other = _blocks(a, b, n, seed + 1)
    right = np.where((np.arange(n) % 2 == 0)[:, None], 0.9 * left + 0.1 * other, other)
    return left, right


def _n_max(a, b):
    return 200 if a + b <= 2048 else 72                      # (the oracle's thresholds cost O(N^2) per block)


def _pieces(n):
    """(start, count) of the calls compared with the whole batch: the few-block encode holds <= 64 blocks (kSmallBatch),
    65 take the batch path"""
    return [(0, 1), (1, 3), (4, 64), (n - 65, 65)]


def _int_keys(joint):
    return ("overall_scale", "bit_alloc", "scale_factor", "mantissa", "reservoir_out") + (("ms_switch",) if joint else ())


def _assert_int_parity(got, ref, joint, what=""):
    for k in _int_keys(joint):
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.shape == r.shape, (what, k, g.shape, r.shape)
        bad = np.argwhere(g != r)
        assert bad.size == 0, "%s %s: %d mismatching entries, first at %s" % (what, k, len(bad), bad[0])


def _cut(ref, i0, i1, joint):
    return {k: np.asarray(ref[k])[i0:i1] for k in _int_keys(joint)}


def _check_rejected(hd, a, b):
    from mrcaudiocodec_amd import MrcError
    assert (a, b) in REFUSED, "the handle refuses (%d,%d)" % (a, b)
    blk = np.zeros((1, a + b))
    for call in (lambda: hd.window(blk, a, b), lambda: hd.mdct(blk, a, b), lambda: hd.smr(blk, a, b),
                 lambda: hd.encode_mono(blk, a, b), lambda: hd.encode_joint(blk, blk, a, b)):
        with pytest.raises(MrcError):
            call()


# ------------------------------------------------------------------ shape tables, window, MDCT, thresholds
@pytest.mark.parametrize("ab", SHAPES)
def test_shape_tables_window_mdct_smr(h, ab):
    a, b = ab
    if not _accepts(h, a, b):
        _check_rejected(h, a, b)
        return
    assert ab not in REFUSED
    half = (a + b) // 2
    sfb = fast.bands_for(a, b)
    assert np.array_equal(h.bands(a, b), np.asarray(sfb.nLines)), ab
    for res in (0, 123, -45):
        assert h.budget(a, b, False, res) == fast.mono_budget(fast.DEFAULTS, half, sfb.nBands) + res
        assert h.budget(a, b, True, res) == fast.joint_budget(fast.DEFAULTS, half, sfb.nBands, res)
    blocks = _blocks(a, b, 24, seed=a + 7 * b)
    # (the library's KBD tables are summed in long double, the oracle's in float64: the oracle's error grows with the
    # window length, 4.4e-16 for KBD(2304))
    assert np.abs(h.window(blocks, a, b) - blocks * fast.transition_table(a, b)).max() <= (4e-16 if max(a, b) <= 1024 else 8e-16)
    X, scale = h.mdct(blocks, a, b)
    ref = fast.mdct_batch(blocks, a, b)
    assert np.abs(X - ref).max() <= MDCT_RTOL * np.abs(ref).max()
    s, Xs = fast.overall_scale_batch(ref, 4)
    assert np.array_equal(scale, s)
    from oracle import mdct as omdct
    X0 = h.mdct(blocks[:1], a, b, apply_window=False)[0][0]
    d = omdct.MDCTslow(blocks[0], a, b)
    assert np.abs(X0 - d).max() <= MDCT_RTOL * np.abs(d).max() * 10
    thr_ref = fast.masked_threshold_batch(blocks, half, 48000)
    smr_ref = fast.smr_batch(blocks, Xs, s, 48000, sfb)
    for exact in (0, 1):
        h.set_option(1, exact)
        try:
            smr, thr = h.smr(blocks, a, b, want_thresh=True)
            smr2 = h.smr(blocks, a, b, scaled_lines=Xs, overall_scale=s)
        finally:
            h.set_option(1, 0)
        assert np.abs(thr - thr_ref).max() <= DB_ATOL, (ab, exact)
        assert np.abs(smr - smr_ref).max() <= DB_ATOL, (ab, exact)
        assert np.abs(smr2 - smr_ref).max() <= DB_ATOL, (ab, exact)


# ------------------------------------------------------------------ whole encode on both sides of the few-block limit, decode
@pytest.mark.parametrize("ab", SHAPES)
def test_encode_and_decode(h, ab):
    a, b = ab
    if not _accepts(h, a, b):
        _check_rejected(h, a, b)
        return
    assert ab not in REFUSED
    n = _n_max(a, b)
    rng = np.random.default_rng(a * 11 + b)
    res_in = rng.integers(-150, 500, n)
    blocks = _blocks(a, b, n, seed=a + b)
    ref = fast.encode_mono_batch(blocks, a, b, res_in)
    whole = h.encode_mono(blocks, a, b, res_in, want_mdct=True)
    _assert_int_parity(whole, _cut(ref, 0, n, False), False, "mono n=%d" % n)
    assert np.abs(whole["mdct"] - ref["mdct"]).max() <= MDCT_RTOL * np.abs(ref["mdct"]).max()
    for i0, m in _pieces(n):                                  # the pieces equal the whole batch bit for bit
        got = h.encode_mono(blocks[i0:i0 + m], a, b, res_in[i0:i0 + m])
        _assert_int_parity(got, _cut(whole, i0, i0 + m, False), False, "mono n=%d" % m)
    left, right = _pair(a, b, n, seed=a + b + 1)
    rj = fast.encode_joint_batch(left, right, a, b, res_in)
    sw = np.asarray(rj["ms_switch"])
    assert sw.any() and not sw.all()                          # both branches of the M/S switch occur
    wj = h.encode_joint(left, right, a, b, res_in, want_mdct=True)
    _assert_int_parity(wj, _cut(rj, 0, n, True), True, "joint n=%d" % n)
    assert np.abs(wj["mdct"] - rj["mdct"]).max() <= MDCT_RTOL * np.abs(rj["mdct"]).max()
    for i0, m in _pieces(n):
        got = h.encode_joint(left[i0:i0 + m], right[i0:i0 + m], a, b, res_in[i0:i0 + m])
        _assert_int_parity(got, _cut(wj, i0, i0 + m, True), True, "joint n=%d" % m)
    # decode of the encoded integers against the oracle's Decode / JointDecode
    cp = ocodec.default_params(nChannels=2)
    cp.a, cp.b, cp.sfBands = a, b, fast.bands_for(a, b)
    k = 4
    dm = h.decode(a, b, whole["overall_scale"][:k], whole["scale_factor"][:k, None], whole["bit_alloc"][:k, None],
                  whole["mantissa"][:k, None])
    dj = h.decode(a, b, wj["overall_scale"][:k], wj["scale_factor"][:k], wj["bit_alloc"][:k], wj["mantissa"][:k],
                  wj["ms_switch"][:k])
    for i in range(k):
        want = odec.Decode(whole["scale_factor"][i], whole["bit_alloc"][i], whole["mantissa"][i],
                           int(whole["overall_scale"][i]), cp)
        assert np.abs(dm[i, 0] - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300), (ab, i)
        want = odec.JointDecode([wj["scale_factor"][i, 0], wj["scale_factor"][i, 1]],
                                [wj["bit_alloc"][i, 0], wj["bit_alloc"][i, 1]],
                                [wj["mantissa"][i, 0], wj["mantissa"][i, 1]], list(wj["overall_scale"][i]), cp,
                                list(wj["ms_switch"][i]))
        for c in range(2):
            assert np.abs(dj[i, c] - want[c]).max() <= 1e-12 * max(np.abs(want[c]).max(), 1e-300), (ab, i, c)


# ------------------------------------------------------------------ codec settings
# Sample rates below about 31 kHz are outside the reference's domain: its band loop (psychoac.py:86-105) runs off the end
# of the frequency-limit table there, so they are not compared.
SETTINGS = [
    dict(n_scale_bits=1),        # (a band without bits has scale factor -1: quantize_kernel must keep it in its byte)
    dict(n_scale_bits=2), dict(n_scale_bits=3),
    dict(n_mant_size_bits=1), dict(n_mant_size_bits=2), dict(n_mant_size_bits=3), dict(n_mant_size_bits=5),
    dict(n_mant_size_bits=8),
    dict(target_bits_per_sample=0.7), dict(target_bits_per_sample=6.5),
    dict(blksw_bits_a=0, blksw_bits_b=0), dict(blksw_bits_a=2, blksw_bits_b=2),
    dict(sample_rate=32000),
    dict(sample_rate=96000),     # (the quiet threshold of the top lines is +inf there: tests/test_gpu_rates.py)
]
_PARAM = dict(sample_rate="sampleRate", n_scale_bits="nScaleBits", n_mant_size_bits="nMantSizeBits",
              target_bits_per_sample="targetBitsPerSample", blksw_bits_a="blkswBitA", blksw_bits_b="blkswBitB")
SETTING_SHAPES = REF_SHAPES + [(576, 576), (162, 162)]


@pytest.mark.parametrize("kw", SETTINGS, ids=lambda kw: "-".join("%s=%s" % kv for kv in kw.items()))
def test_codec_settings(kw):
    from mrcaudiocodec_amd import Handle
    params = {_PARAM[k]: v for k, v in kw.items()}
    sr = kw.get("sample_rate", 48000)
    hd = Handle(device_id=0, **kw)
    try:
        for (a, b) in SETTING_SHAPES:
            sfb = fast.bands_for(a, b, 1024, sr)
            assert np.array_equal(hd.bands(a, b), np.asarray(sfb.nLines)), (kw, a, b)
            n = 72
            res_in = np.random.default_rng(a + b).integers(-100, 300, n)
            blocks = _blocks(a, b, n, seed=3 * a + b)
            ref = fast.encode_mono_batch(blocks, a, b, res_in, params=params)
            _assert_int_parity(hd.encode_mono(blocks, a, b, res_in), ref, False, "%s %s mono" % (kw, (a, b)))
            _assert_int_parity(hd.encode_mono(blocks[:5], a, b, res_in[:5]), _cut(ref, 0, 5, False), False,
                               "%s %s mono n=5" % (kw, (a, b)))
            if (a, b) not in ((1024, 1024), (128, 128), (576, 576)):
                continue
            left, right = _pair(a, b, n, seed=a + 2 * b)
            rj = fast.encode_joint_batch(left, right, a, b, res_in, params=params)
            _assert_int_parity(hd.encode_joint(left, right, a, b, res_in), rj, True, "%s %s joint" % (kw, (a, b)))
            _assert_int_parity(hd.encode_joint(left[:5], right[:5], a, b, res_in[:5]), _cut(rj, 0, 5, True), True,
                               "%s %s joint n=5" % (kw, (a, b)))
    finally:
        hd.close()


# ------------------------------------------------------------------ block switching with other block sizes
def _switched_stream(L, S, hops, seed):
    """a stereo stream [2][(hops + 1) L] (leading zero hop) with bursts, and its block shapes: every fourth hop is coded
    as L/S short blocks, with the transitions (L,S) and (S,L) around it"""
    from mrcaudiocodec_amd import synth
    rng = np.random.default_rng(seed)
    g = rng.normal(0, 0.02 * 32767, (2, hops * L))
    shapes, off, a = [], 0, L
    for k in range(hops):
        if k % 4 == 2:
            g[:, k * L:k * L + S] += rng.normal(0, 0.4 * 32767, (2, S))
            for _ in range(L // S):
                shapes.append((off, a, S)); off += a; a = S
        else:
            shapes.append((off, a, L)); off += a; a = L
    g[1] = 0.7 * g[0] + 0.3 * g[1]
    x = np.concatenate([np.zeros((2, L)), synth.pcm_to_float(np.clip(np.rint(g), -32767, 32767))], axis=1)
    return x, shapes


@pytest.mark.parametrize("huff", [True, False])
def test_block_switching_512_256(huff):
    from mrcaudiocodec_amd import Handle, pacfile as ppac
    from oracle import pacfile as opac
    L, S = 512, 256
    hd = Handle(device_id=0, n_mdct_lines=L, n_short=S)
    try:
        stream, shapes = _switched_stream(L, S, hops=14, seed=5)
        assert {(a, b) for (_, a, b) in shapes} == {(L, L), (L, S), (S, S), (S, L)} and shapes[-1][2] == L
        for (a, b) in ((L, L), (L, S), (S, S), (S, L)):
            assert np.array_equal(hd.bands(a, b), np.asarray(fast.bands_for(a, b, L).nLines)), (a, b)
        cp = ocodec.default_params(nChannels=2)
        cp.nMDCTLines = cp.nSamplesPerBlock = cp.a = cp.b = L
        cp.nSamplesShort = S
        cp.sfBands = ocodec.bands_for_block(L, L, L, cp.sampleRate)
        want = opac.encode_stereo_stream(stream, shapes, cp=cp, huffman=huff)
        got = ppac.encode_stereo_stream(hd, stream, shapes, use_huffman=huff)
        assert got == want
        assert ppac.encode_stereo_stream_per_block(hd, stream, shapes, use_huffman=huff) == want
    finally:
        hd.close()


def test_chained_refuses_joint_blocks_of_more_than_2048_lines():
    from mrcaudiocodec_amd import Handle, MrcError
    L, S = 2048, 256
    stream, shapes = _switched_stream(L, S, hops=3, seed=9)
    try:
        hd = Handle(device_id=0, n_mdct_lines=L, n_short=S)
    except MrcError:
        return                               # (refused already: the long block is too long for the masking model)
    try:
        with pytest.raises(MrcError) as e:
            hd.encode_chained_pac(stream[0][None], stream[1][None], [shapes])
        if _accepts(hd, L, L):
            assert "2048 coded lines" in str(e.value)
    finally:
        hd.close()


# ------------------------------------------------------------------ alignment fallbacks of the device entry point
@pytest.mark.parametrize("ab", REF_SHAPES + [(576, 576), (162, 162)])
def test_dev_encode_unaligned_outputs(h, ab):
    torch = pytest.importorskip("torch")
    from mrcaudiocodec_amd import synth
    a, b = ab
    n, half, nb = 70, (a + b) // 2, len(h.bands(a, b))
    dev = "cuda:0"
    rng = np.random.default_rng(a + 3 * b)
    pcm = [np.clip(np.rint(rng.normal(0, 0.1 * 32767, n * (a + b))), -32767, 32767).astype(np.int16) for _ in range(2)]
    pcm[1] = np.clip(np.rint(0.8 * pcm[0] + 0.2 * pcm[1]), -32767, 32767).astype(np.int16)
    pcm[1][: n // 2 * (a + b)] = pcm[1][: n // 2 * (a + b)][::-1]            # half the pairs unrelated
    res_in = rng.integers(-100, 300, n).astype(np.int32)
    res_d = torch.from_numpy(res_in).to(dev)
    fl = [synth.pcm_to_float(p).reshape(n, a + b) for p in pcm]
    refs = {False: fast.encode_mono_batch(fl[0], a, b, res_in), True: fast.encode_joint_batch(fl[0], fl[1], a, b, res_in)}

    def run(joint, fmt, mfmt, shift):
        src = [torch.from_numpy(p).to(dev) if fmt == 1 else torch.from_numpy(synth.pcm_to_float(p)).to(dev) for p in pcm]
        nsig, ns = (4, 2) if joint else (1, 1)
        mdt = torch.int16 if mfmt == 1 else torch.int32
        mstep = 8 // (2 if mfmt == 1 else 4)                  # 8 bytes in elements
        lines_buf = torch.empty(n * nsig * half + 2, dtype=torch.float64, device=dev)
        mant_buf = torch.empty(n * ns * half + 8, dtype=mdt, device=dev)
        assert lines_buf.data_ptr() % 16 == 0 and mant_buf.data_ptr() % 16 == 0
        lines = lines_buf[1:1 + n * nsig * half] if shift else lines_buf[:n * nsig * half]
        mant = mant_buf[mstep:mstep + n * ns * half] if shift else mant_buf[:n * ns * half]
        osc = torch.empty(n * nsig, dtype=torch.int32, device=dev)
        sw = torch.empty(n * nb, dtype=torch.int32, device=dev)
        ba = torch.empty(n * ns * nb, dtype=torch.int32, device=dev)
        sf = torch.empty_like(ba)
        ro = torch.empty(n, dtype=torch.int32, device=dev)
        h.dev_encode_ex(a, b, n, src[0].data_ptr(), src[1].data_ptr() if joint else None, fmt, a + b, None,
                        res_d.data_ptr(), osc.data_ptr(), sw.data_ptr() if joint else None, ba.data_ptr(), sf.data_ptr(),
                        mant.data_ptr(), mfmt, ro.data_ptr(), lines.data_ptr())
        torch.cuda.synchronize()
        out = dict(overall_scale=osc.cpu().numpy().reshape((n, 4) if joint else (n,)),
                   bit_alloc=ba.cpu().numpy().reshape((n, 2, nb) if joint else (n, nb)),
                   scale_factor=sf.cpu().numpy().reshape((n, 2, nb) if joint else (n, nb)),
                   mantissa=mant.cpu().numpy().astype(np.int64) & (0xFFFF if mfmt == 1 else -1),
                   reservoir_out=ro.cpu().numpy(), lines=lines.cpu().numpy().reshape(n, nsig, half))
        out["mantissa"] = out["mantissa"].reshape((n, 2, half) if joint else (n, half))
        if joint:
            out["ms_switch"] = sw.cpu().numpy().reshape(n, nb)
        return out

    for joint in (False, True):
        ref = refs[joint]
        X = np.asarray(ref["mdct"]).reshape(n, -1, half)
        for fmt in (0, 1):                                    # MRC_SAMPLES_F64, MRC_SAMPLES_PCM16
            for mfmt in (0, 1):                               # MRC_MANTISSA_I32, MRC_MANTISSA_I16
                al = run(joint, fmt, mfmt, False)
                un = run(joint, fmt, mfmt, True)
                what = "%s joint=%d fmt=%d mfmt=%d" % (ab, joint, fmt, mfmt)
                _assert_int_parity(al, ref, joint, what + " aligned")
                _assert_int_parity(un, al, joint, what + " unaligned")
                # (the lines themselves come from another transform kernel when unaligned: equal to the oracle's within
                # the MDCT bar, not bit for bit to the aligned call's)
                assert np.abs(un["lines"] - X).max() <= MDCT_RTOL * np.abs(X).max(), what
