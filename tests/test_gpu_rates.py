"""
GPU parity at sample rates other than 48 kHz: 32, 44.1, 88.2, 96 and 192 kHz, on the reference's block shapes and (576,576),
against the oracle and against the reference's own outputs (tests/golden/ref_rates*.npz, ref_pac_rates.npz).

What changes with the rate: binHz = fs // N (Python-2 integer division), the line centres, the Bark grid, the quiet
threshold -- whose intensity overflows to +inf on the top lines from ~80 kHz on (the reference's own values) -- and the
transient detector's cheby2(20, 40, 9000/fs), unstable as the reference builds it from 88.2 kHz on.  Content puts peaks
and maskers in the overflowing region.  Thresholds are compared with non-finite values handled explicitly (same +-inf
positions, no NaN, finite values within 1e-9 dB); every integer of an encode is compared bit for bit.
"""
import numpy as np
import pytest

import refgold as G
from oracle import codec as ocodec, fast, pacfile as opac, transient as otr
from test_gpu_shapes import _assert_int_parity, _cut
from test_rates_golden import assert_same_nonfinite

pytestmark = pytest.mark.gpu

RATES = (32000, 44100, 88200, 96000, 192000)
SHAPES = [(1024, 1024), (128, 128), (1024, 128), (128, 1024), (576, 576)]
DB_ATOL = 1e-9
ERR = dict(over="ignore", divide="ignore", invalid="ignore")


def _defined(a, b, fs):
    """the reference computes SMRs only where no band is empty (192 kHz (128,128) has two empty bands:
    CalcSMRs' np.amax over nothing raises)"""
    return min(fast.bands_for(a, b, 1024, fs).nLines) > 0


@pytest.fixture(scope="module", params=RATES, ids=lambda r: "%dHz" % r)
def hr(request):
    from mrcaudiocodec_amd import Handle
    hd = Handle(device_id=0, sample_rate=request.param)
    yield hd, request.param
    hd.close()


def _blocks(a, b, n, fs, seed):
    """n blocks of 16-bit content: noise of changing level up to Nyquist, tones at 30 / 40 / 45 kHz where the rate has
    them, a tone just below the first line whose quiet threshold is +inf, and a silent block"""
    from mrcaudiocodec_amd import synth
    rng = np.random.default_rng(seed)
    N = a + b
    half = N // 2
    f = (np.arange(half) + 0.5) * ((float(fs) / half) / 2.)
    with np.errstate(**ERR):
        inf = np.flatnonzero(np.isinf(10 ** ((ocodec_thresh(f) - 96) / 10)))
    f_top = (f[inf[0]] if len(inf) else f[-1]) - 0.75 * fs / N
    t = np.arange(N)[None, :] + np.arange(n)[:, None] * b
    sigma = rng.choice([0.003, 0.03, 0.1, 0.4], size=n)[:, None]
    x = rng.normal(0, 1, (n, N)) * sigma
    tones = sum(0.15 * np.sin(2 * np.pi * fr / fs * t + 0.3) for fr in (30000.0, 40000.0, 45000.0) if fr < 0.45 * fs)
    kind = np.arange(n) % 4
    x = np.where((kind == 1)[:, None], x * 0.1 + tones, x)
    x = np.where((kind == 2)[:, None], x * 0.1 + 0.3 * np.sin(2 * np.pi * f_top / fs * t), x)
    x[n // 2] = 0.0                                                          # digital silence
    return synth.pcm_to_float(np.clip(np.rint(x * 32767), -32767, 32767))


def ocodec_thresh(f):
    from oracle import psychoac
    return psychoac.Thresh(f)


# ------------------------------------------------------------------ band tables, thresholds, SMRs
def test_bands_at_every_rate(hr):
    h, fs = hr
    for (a, b) in SHAPES + [(162, 162)]:
        assert np.array_equal(h.bands(a, b), np.asarray(fast.bands_for(a, b, 1024, fs).nLines)), (fs, a, b)


@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
def test_thresholds_and_smrs_at_every_rate(hr, exact):
    h, fs = hr
    h.set_option(1, 1 if exact else 0)                                     # MRC_OPT_EXACT_SPREAD
    try:
        for (a, b) in SHAPES:
            n = 12
            blocks = _blocks(a, b, n, fs, seed=a + 3 * b + fs)
            half = (a + b) // 2
            with np.errstate(**ERR):
                thr_ref = fast.masked_threshold_batch(blocks, half, fs)
            smr, thr = h.smr(blocks, a, b, want_thresh=True)
            smr_only = h.smr(blocks, a, b)                                   # (the ratio form: no per-line thresholds)
            what = "%d Hz %s %s" % (fs, (a, b), "exact" if exact else "fast")
            assert_same_nonfinite(thr, thr_ref, DB_ATOL, what + " thresholds")
            if fs >= 88200 and half >= 128:
                assert np.isinf(thr_ref).any(), what
            if not _defined(a, b, fs):
                continue
            sfb = fast.bands_for(a, b, 1024, fs)
            X = fast.mdct_batch(blocks, a, b)
            s, Xs = fast.overall_scale_batch(X, 4)
            with np.errstate(**ERR):
                smr_ref = fast.smr_batch(blocks, Xs, s, fs, sfb)
            assert_same_nonfinite(smr, smr_ref, DB_ATOL, what + " SMRs (with thresholds)")
            assert_same_nonfinite(smr_only, smr_ref, DB_ATOL, what + " SMRs")
            assert np.isfinite(smr_ref[np.arange(n) != n // 2]).all(), what
    finally:
        h.set_option(1, 0)


@pytest.mark.parametrize("fs", (32000, 88200, 96000, 192000))
def test_thresholds_and_smrs_equal_reference_fixture(fs):
    from mrcaudiocodec_amd import Handle
    s = G.load("ref_rates_smr.npz")
    h = Handle(device_id=0, sample_rate=fs)
    try:
        for (a, b) in SHAPES[:4]:
            key = "%d_%d_%d" % (a, b, fs)
            blocks = np.array([G.pcm_to_float(p) for p in s["pcm_" + key]])
            smr, thr = h.smr(blocks, a, b, want_thresh=True)
            assert_same_nonfinite(thr, s["thr_" + key], DB_ATOL, key)
            if ("smr_" + key) in s.files:
                assert_same_nonfinite(smr, s["smr_" + key], DB_ATOL, key)
                assert_same_nonfinite(h.smr(blocks, a, b), s["smr_" + key], DB_ATOL, key + " (ratio form)")
    finally:
        h.close()


# ------------------------------------------------------------------ encode
def test_encode_at_every_rate(hr):
    """mono and joint at n = 72 (batch path), 5 and 1 (the few-block chained back end), every integer bit for bit"""
    h, fs = hr
    params = dict(sampleRate=fs)
    for (a, b) in SHAPES:
        if not _defined(a, b, fs):
            continue
        n = 72
        res_in = np.random.default_rng(a + b).integers(-100, 300, n)
        blocks = _blocks(a, b, n, fs, seed=5 * a + b)
        with np.errstate(**ERR):
            ref = fast.encode_mono_batch(blocks, a, b, res_in, params=params)
        for m in (n, 5, 1):
            _assert_int_parity(h.encode_mono(blocks[:m], a, b, res_in[:m]), _cut(ref, 0, m, False), False,
                               "%d Hz %s mono n=%d" % (fs, (a, b), m))
        other = _blocks(a, b, n, fs, seed=7 * a + b)
        right = np.where((np.arange(n) % 2 == 0)[:, None], 0.9 * blocks + 0.1 * other, other)
        with np.errstate(**ERR):
            rj = fast.encode_joint_batch(blocks, right, a, b, res_in, params=params)
        for m in (n, 5, 1):
            _assert_int_parity(h.encode_joint(blocks[:m], right[:m], a, b, res_in[:m]), _cut(rj, 0, m, True), True,
                               "%d Hz %s joint n=%d" % (fs, (a, b), m))


@pytest.mark.parametrize("tag,joint", [("r96long", False), ("r96single", False), ("r96jointch", True),
                                       ("r96jointlong", True), ("r32single", False), ("r32jointch", True)])
def test_encode_chains_equal_reference_fixture(tag, joint):
    """the reference's EncodeSingleChannel / JointEncodeChannels chains (reservoir carried), block by block"""
    from mrcaudiocodec_amd import Handle
    r = G.load("ref_rates.npz")
    fs = int(r[tag + "_params"][0])
    h = Handle(device_id=0, sample_rate=fs)
    try:
        for i, (a, b, full) in enumerate(G.blocks_of(r, tag)):
            k = "%s_%d" % (tag, i)
            res = np.array([int(r[tag + "_res_in"][i])])
            if joint:
                got = h.encode_joint(full[0][None], full[1][None], a, b, res)
                assert np.array_equal(got["ms_switch"][0], r[k + "_ms"]), k
                assert np.array_equal(got["mantissa"][0, 0], r[k + "_mant0"]), k
                assert np.array_equal(got["mantissa"][0, 1], r[k + "_mant1"]), k
                assert np.array_equal(got["bit_alloc"][0], r[k + "_ba"]) and np.array_equal(got["scale_factor"][0], r[k + "_sf"]), k
                assert np.array_equal(got["overall_scale"][0], r[k + "_os"]), k
            else:
                got = h.encode_mono(full[0][None], a, b, res)
                assert np.array_equal(got["mantissa"][0], r[k + "_mant0"]), k
                assert np.array_equal(got["bit_alloc"][0], r[k + "_ba"][0]), k
                assert np.array_equal(got["scale_factor"][0], r[k + "_sf"][0]), k
                assert int(got["overall_scale"][0]) == int(r[k + "_os"][0]), k
            assert int(got["reservoir_out"][0]) == int(r[tag + "_res_out"][i]), k
    finally:
        h.close()


# ------------------------------------------------------------------ chained .pac encode
def _stream(hops, fs, seed, n_ch=2):
    from mrcaudiocodec_amd import synth
    rng = np.random.default_rng(seed)
    t = np.arange(hops * 1024)
    g = rng.normal(0, 0.05 * 32767, (n_ch, hops * 1024)) + 4000 * np.sin(2 * np.pi * min(30000.0, 0.4 * fs) / fs * t)
    if n_ch == 2:
        g[1] = 0.7 * g[0] + 0.3 * g[1]
    x = synth.pcm_to_float(np.clip(np.rint(g), -32767, 32767))
    return np.concatenate([np.zeros((n_ch, 1024)), x], axis=1)


def _schedules(hops):
    long_only = [(i * 1024, 1024, 1024) for i in range(hops)]
    sw, off, a = [], 0, 1024
    for k in range(hops):
        if k % 4 == 2 and k < hops - 1:
            for _ in range(8):
                sw.append((off, a, 128)); off += a; a = 128
        else:
            sw.append((off, a, 1024)); off += a; a = 1024
    return {"long": long_only, "switched": sw}


@pytest.mark.parametrize("huff", [True, False], ids=["huffman", "raw"])
def test_chained_pac_at_every_rate(hr, huff):
    from mrcaudiocodec_amd import pacfile as ppac
    import mono_oracle as MO
    h, fs = hr
    hops = 7
    st = _stream(hops, fs, seed=fs // 100)
    mono = _stream(hops, fs, seed=fs // 100 + 1, n_ch=1)
    for name, shapes in _schedules(hops).items():
        if name == "switched" and not _defined(128, 128, fs):
            continue
        cp = ocodec.default_params(sampleRate=fs, nChannels=2)
        with np.errstate(**ERR):
            want = opac.encode_stereo_stream(st, shapes, cp=cp, huffman=huff)
        assert ppac.encode_stereo_stream(h, st, shapes, use_huffman=huff) == want, (fs, name)
        assert ppac.encode_stereo_stream_per_block(h, st, shapes, use_huffman=huff) == want, (fs, name)
        cp1 = ocodec.default_params(sampleRate=fs, nChannels=1)
        with np.errstate(**ERR):
            want1 = MO.encode_mono_stream(mono, shapes, cp=cp1, huffman=huff)
        assert ppac.encode_mono_stream(h, mono, shapes, use_huffman=huff) == want1, (fs, name)
        assert ppac.encode_mono_stream_per_block(h, mono, shapes, use_huffman=huff) == want1, (fs, name)


# ------------------------------------------------------------------ the reference's own files
@pytest.mark.parametrize("case", ["s32", "s96"])
def test_cli_bytes_and_decode_equal_reference_files(tmp_path, case):
    from mrcaudiocodec_amd import Handle, cli, pacfile as ppac
    g = G.load("ref_pac_rates.npz")
    pcm, rate = g[case + "_pcm"], int(g[case + "_rate"])
    wav = str(tmp_path / "in.wav")
    with open(wav, "wb") as f:
        f.write(cli.wav_bytes(pcm, rate))
    assert cli.encode_wav(wav, None) == g[case + "_pac"].tobytes()
    want = g[case + "_decoded"]             # its first 1024 samples are the reference driver's stale look-ahead block
    h = Handle(device_id=0, sample_rate=rate)
    try:
        got = ppac.decode_pac_files(h, [g[case + "_pac"].tobytes()])[0]
    finally:
        h.close()
    assert np.array_equal(got[:, :want.shape[1] - 1024], want[:, 1024:])
    pac = str(tmp_path / "in.pac")
    with open(pac, "wb") as f:
        f.write(g[case + "_pac"].tobytes())
    got = cli.decode_pac_file(pac, str(tmp_path / "out.wav"))                # cli -d
    assert np.array_equal(got[:, :want.shape[1] - 1024], want[:, 1024:])


def test_cli_mono_96k_equals_reference_file(tmp_path):
    import mono_oracle as MO
    from mrcaudiocodec_amd import cli
    g = G.load("ref_pac_rates.npz")
    wav = str(tmp_path / "m.wav")
    with open(wav, "wb") as f:
        f.write(MO.wav_bytes(g["m96_pcm"], 96000))
    assert cli.encode_wav(wav, None) == g["m96_pac"].tobytes()


def test_detector_at_every_rate(hr):
    """transient_peaks with the reference's filter against sosfilt -- from 88.2 kHz on the filter is unstable and the
    peaks grow to ~1e114 within a hop -- and the block shapes against the oracle's"""
    from mrcaudiocodec_amd import transient as ptr
    from test_transient import _scipy_peaks
    h, fs = hr
    s = _stream(16, fs, seed=3)
    sos = otr.design_sos(fs)
    assert np.array_equal(sos, ptr.design_sos(fs))
    got = h.transient_peaks(s, sos)
    with np.errstate(**ERR):
        want = _scipy_peaks(s, sos)
    assert np.isfinite(want).all()
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), fs
    if fs >= 88200:
        assert want.max() > 1e60
    with np.errstate(**ERR):
        ref_shapes = otr.block_shapes(s, ocodec.default_params(sampleRate=fs, nChannels=2), sos)
    assert ptr.block_shapes(h, s, sos) == ref_shapes
    if fs >= 88200:
        assert sum(b == 128 for (_o, _a, b) in ref_shapes) > 8 * 12          # the degenerate schedule
    with np.errstate(**ERR):
        ref_m = otr.block_shapes(s[:1], ocodec.default_params(sampleRate=fs, nChannels=1), sos)
    assert ptr.block_shapes(h, s[:1], sos) == ref_m


def test_sensitivity_at_every_rate(hr):
    h, fs = hr
    h.set_option(5, 1)                                                     # MRC_OPT_SENSITIVITY
    try:
        h.sensitivity()
        shapes = _schedules(7)["long"]
        st = _stream(7, fs, seed=9)
        h.encode_chained_pac(st[0][None], st[1][None], [shapes])
        h.encode_chained_pac(st[0][None], None, [shapes])
        c = h.sensitivity()
        assert c["blocks_examined"] > 0, c
        assert all(np.isfinite(v) and 0 <= v < 2 ** 62 for v in c.values()), c
        near = sum(c[k] for k in ("quantiser_edges", "bitalloc_near_ties", "ms_switch_near_threshold", "peak_near_ties"))
        assert near == 0, (fs, c)
    finally:
        h.set_option(5, 0)


# ------------------------------------------------------------------ the domain: below ~31 kHz the reference raises
@pytest.mark.parametrize("shape,lowest", [((1024, 1024), 31016), ((1024, 128), 31027), ((576, 576), 31027),
                                          ((162, 162), 31096), ((128, 128), 31122)])
def test_handle_refuses_rates_below_the_domain(shape, lowest):
    """shape by shape through a handle whose own shapes are all (1024,1024) (defined from 31016 Hz on): r* accepted,
    r* - 1 refused with the rate named; and mrc_create itself for the handle's long and short shapes"""
    from mrcaudiocodec_amd import Handle, MrcError
    for rate in (lowest, lowest - 1):
        if rate < 31016:
            with pytest.raises(MrcError, match="sample rate %d Hz" % rate):
                Handle(device_id=0, sample_rate=rate, n_short=1024)
            continue
        h = Handle(device_id=0, sample_rate=rate, n_short=1024)
        try:
            if rate == lowest:
                assert np.array_equal(h.bands(*shape), np.asarray(fast.bands_for(*shape, 1024, rate).nLines))
                _assert_int_parity(h.encode_mono(np.zeros((1, sum(shape))), *shape),
                                   fast.encode_mono_batch(np.zeros((1, sum(shape))), *shape, params=dict(sampleRate=rate)),
                                   False, "%s at %d Hz" % (shape, rate))
            else:
                with pytest.raises(MrcError, match="sample rate %d Hz" % rate):
                    h.bands(*shape)
                with pytest.raises(MrcError, match="sample rate %d Hz" % rate):
                    h.encode_mono(np.zeros((1, sum(shape))), *shape)
        finally:
            h.close()
    if shape == (128, 128):                                                # the default handle: its short shape
        Handle(device_id=0, sample_rate=lowest).close()
        with pytest.raises(MrcError, match="sample rate %d Hz is outside .* \\(128,128\\)" % (lowest - 1)):
            Handle(device_id=0, sample_rate=lowest - 1)


def test_cli_and_decoder_refuse_rates_below_the_domain(tmp_path):
    from mrcaudiocodec_amd import Handle, MrcError, cli, pacfile as ppac
    rng = np.random.default_rng(4)
    pcm = np.clip(np.rint(rng.normal(0, 3000, (2, 5 * 1024))), -32767, 32767).astype(np.int16)
    for rate in (22050, 31121):
        wav = str(tmp_path / ("r%d.wav" % rate))
        with open(wav, "wb") as f:
            f.write(cli.wav_bytes(pcm, rate))
        with pytest.raises(ValueError, match="%d Hz" % rate):
            cli.encode_wav(wav, None)
    wav = str(tmp_path / "ok.wav")
    with open(wav, "wb") as f:
        f.write(cli.wav_bytes(pcm, 31122))
    data = cli.encode_wav(wav, None)
    assert data == opac.encode_wav(wav, huffman=True)
    bad = bytearray(data)
    bad[4:8] = (31015).to_bytes(4, "little")
    with pytest.raises(MrcError, match="sample rate 31015 Hz"):
        ppac.read_header(bytes(bad))
    h = Handle(device_id=0, sample_rate=31122)
    try:
        with pytest.raises(MrcError, match="sample rate 31015 Hz"):
            ppac.decode_pac_files(h, [bytes(bad)])
    finally:
        h.close()
