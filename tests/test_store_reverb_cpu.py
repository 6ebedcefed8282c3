"""
The store's reverberated windows (mrc_pac_store_set_irs, mrc_pac_store_decode_window_reverb, PacStore.set_impulse_responses /
decode_window(ir_index=) / decode_window_sum(ir_index=), store.ir_at_rate, cli -d --ir) as far as a CPU reaches: the binding
against the header; the Python-side refusals, raised before any library call; ir_at_rate -- identity at equal rates, the DC
gain, the length rule, and a direct NumPy restatement of the polyphase fold; the error measure of the GPU test's tolerance; the
command line's argument checks.
"""
import numpy as np
import pytest

import chain_kit as kit
import reverb_reference as RV


# ------------------------------------------------------------------ the binding
def test_binding_of_the_reverb_calls():
    from mrcaudiocodec_amd import _lib, store
    names = ("mrc_pac_store_set_irs", "mrc_pac_store_ir_info", "mrc_pac_store_decode_window_reverb", "mrc_pac_store_reverb_ms")
    kit.check_binding(names)
    assert all(hasattr(_lib.lib, n) for n in names)
    args = [a.split()[-1].lstrip("*") for a in kit.header_args("mrc_pac_store_decode_window_reverb")]
    speeds = [a.split()[-1].lstrip("*") for a in kit.header_args("mrc_pac_store_decode_window_speeds")]
    assert [n for n in args if n != "ir_of"] == speeds and args.index("ir_of") == args.index("ratio_of") + 1
    assert [a.split()[-1].lstrip("*") for a in kit.header_args("mrc_pac_store_set_irs")] == ["s", "n_irs", "ir_offset", "taps"]
    text = kit.header_text()
    assert "#define MRC_STORE_REVERB_BLOCK %d" % _lib.MRC_STORE_REVERB_BLOCK in text and _lib.MRC_STORE_REVERB_BLOCK == 1024
    assert "#define MRC_MAX_STORE_IR_TAPS (1 << 17)" in text and _lib.MRC_MAX_STORE_IR_TAPS == 1 << 17
    assert store.REVERB_BLOCK == 1024 and store.MAX_IR_TAPS == 1 << 17


# ------------------------------------------------------------------ Python-side checks
def _husk(monkeypatch, n_irs=3):
    import store_kit
    return store_kit.husk(monkeypatch, n_irs=n_irs)


@pytest.mark.parametrize("ir_index,text", [
    ([0], r"ir_index must have shape \(2,\), got \(1,\)"),
    ([[0, 1]], r"ir_index must have shape \(2,\)"),
    ([0, 3], r"ir_index must be -1 or lie in 0\.\.2 .* got 3 at unit 1"),
    ([-2, 0], r"ir_index must be -1 or lie in 0\.\.2 .* got -2 at unit 0"),
    ([0.0, 1.0], "ir_index must be ints"),
    (["a", "b"], "ir_index must be ints"),
])
def test_bad_ir_indices_are_refused_before_any_library_call(monkeypatch, ir_index, text):
    pytest.importorskip("torch")
    s = _husk(monkeypatch)
    with pytest.raises(ValueError, match="decode_window: .*" + text):
        s.decode_window([0, 1], [0, 5], 16, ir_index=ir_index)
    text = text.replace(r"\(2,\)", r"\(1, 2\)").replace(r"got \(1,\)", r"got \(1, 1\)")
    with pytest.raises(ValueError, match="decode_window_sum: .*" + text):
        s.decode_window_sum([[0, 1]], [[0, 5]], [[1.0, 0.5]], 16, ir_index=[ir_index])
    # ... and the neighbours' own refusals still come first or alongside
    with pytest.raises(ValueError, match="speed_factors and speed_index go together"):
        s.decode_window([0, 1], [0, 5], 16, ir_index=[0, -1], speed_factors=[(1, 1)])


def test_an_index_without_a_bank_is_refused_before_any_library_call(monkeypatch):
    pytest.importorskip("torch")
    s = _husk(monkeypatch, n_irs=0)
    with pytest.raises(ValueError, match=r"decode_window: ir_index names impulse response 0 at unit 1, but the store has none"):
        s.decode_window([0, 1], [0, 5], 16, ir_index=[-1, 0])
    with pytest.raises(ValueError, match=r"decode_window_sum: ir_index names impulse response 2 at unit 0"):
        s.decode_window_sum([[0, 1]], [[0, 5]], [[1.0, 0.5]], 16, ir_index=[[2, -1]])
    assert s.impulse_response_lengths.size == 0


def test_check_impulse_responses(monkeypatch):
    from mrcaudiocodec_amd.store import MAX_IR_TAPS, check_impulse_responses, check_ir_index
    offsets, taps = check_impulse_responses([[1.0, 0.5], np.arange(3, dtype=np.int16), np.float32([0.25])])
    assert offsets.dtype == np.int64 and offsets.tolist() == [0, 2, 5, 6] and taps.dtype == np.float64
    assert taps.tolist() == [1.0, 0.5, 0.0, 1.0, 2.0, 0.25] and taps.flags.c_contiguous
    for none in (None, [], ()):
        offsets, taps = check_impulse_responses(none)
        assert offsets.tolist() == [0] and taps.size == 0
    assert check_impulse_responses([np.zeros(MAX_IR_TAPS)])[0].tolist() == [0, MAX_IR_TAPS]
    for bad, text in ((np.zeros(4), "must be a list of 1-D arrays"), ("room.npy", "must be a list of 1-D arrays"), ([[]], "impulse response 0 must be 1-D with 1 to"),
                      ([[1.0], np.zeros((2, 2))], "impulse response 1 must be 1-D"), ([np.zeros(MAX_IR_TAPS + 1)], "impulse response 0 must be 1-D with 1 to 131072"),
                      ([[1.0, float("nan")]], r"impulse response 0 must be finite, got nan at tap 1"), ([[1.0], [float("inf")]], "impulse response 1 must be finite"),
                      ([["a"]], "impulse response 0 must be numbers"), ([[1.0], None], "impulse response 1 must be numbers")):
        with pytest.raises(ValueError, match="set_impulse_responses: .*" + text):
            check_impulse_responses(bad)
    s = _husk(monkeypatch)
    with pytest.raises(ValueError, match="set_impulse_responses: impulse response 0 must be finite"):
        s.set_impulse_responses([[float("nan")]])                    # before any library call
    i = check_ir_index([[0, -1], [2, 1]], (2, 2), 3, "f")
    assert i.dtype == np.int32 and i.flags.c_contiguous and i.tolist() == [0, -1, 2, 1]
    assert check_ir_index(np.zeros(0, np.int64), (0,), 0, "f").shape == (0,)
    assert check_ir_index([-1, -1], (2,), 0, "f").tolist() == [-1, -1]


# ------------------------------------------------------------------ ir_at_rate
def _restated(ir, up, down):
    """the polyphase fold said directly, sample by sample: output n at input time n down / up"""
    from mrcaudiocodec_amd.store import resample_taps
    W, taps = resample_taps(up, down)
    n_out = -(-len(ir) * up // down)
    out = np.zeros(n_out)
    for n in range(n_out):
        q, p = (n * down) // up, (n * down) % up
        acc = 0.0
        for j in range(2 * W):
            m = q - W + 1 + j
            if 0 <= m < len(ir):
                acc += taps[p][j] * ir[m]
        out[n] = acc * (down / up)
    return out


@pytest.mark.parametrize("rate_in,rate_out", [(48000, 16000), (16000, 48000), (44100, 16000), (32000, 48000), (48000, 44100)])
def test_ir_at_rate(rate_in, rate_out):
    from mrcaudiocodec_amd.store import ir_at_rate
    ir = RV.room(331, 5)
    got = ir_at_rate(ir, rate_in, rate_out)
    g = int(np.gcd(rate_in, rate_out))
    up, down = rate_out // g, rate_in // g
    assert got.dtype == np.float64 and got.shape == (-(-331 * up // down),)                    # the length rule
    assert abs(got.sum() - ir.sum()) <= 1e-12 * np.abs(ir).sum()                               # the DC gain
    want = _restated(ir, up, down)
    assert abs(want.sum() - ir.sum()) <= 0.5 * abs(ir.sum())                                   # (the nominal factor is close ...)
    want *= ir.sum() / want.sum()                                                              # (... and the rescale is exact)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(ir).max()


def test_ir_at_rate_identity_and_refusals():
    from mrcaudiocodec_amd.store import ir_at_rate
    ir = RV.room(100, 1)
    for rate in (16000, 48000):
        same = ir_at_rate(ir, rate, rate)
        assert np.array_equal(same, ir) and same is not ir and same.dtype == np.float64
    assert np.array_equal(ir_at_rate(np.float32([1, 0.5]), 8000, 8000), [1.0, 0.5])
    assert np.array_equal(ir_at_rate([0.0, 0.0], 48000, 16000), [0.0])                         # a sum of zero: no rescale
    for kw, text in ((dict(rate_in=0), "rate_in must be a positive int"), (dict(rate_out=16000.0), "rate_out must be a positive int"),
                     (dict(rate_in=True), "rate_in must be a positive int"), (dict(ir=[[1.0, 2.0]]), "must be 1-D"),
                     (dict(ir=[float("nan")]), "must be finite"), (dict(ir=[]), "must be 1-D with 1 to"),
                     (dict(rate_in=48000, rate_out=4000), "up / down = 1 / 12 is outside"), (dict(rate_in=48000, rate_out=47999), "is above 1024")):
        a = dict(ir=ir, rate_in=48000, rate_out=16000)
        a.update(kw)
        with pytest.raises(ValueError, match="ir_at_rate: .*" + text):
            ir_at_rate(**a)


# ------------------------------------------------------------------ the GPU test's error measure
def test_the_reference_and_the_error_scale():
    rng = np.random.default_rng(0)
    worst = 0.0
    for window, L in ((1, 1), (257, 2), (1025, 1023), (300, 3089), (2049, 1)):
        h, w = RV.room(L, L), rng.standard_normal(window + L - 1)
        ref = RV.wet_reference(h, w)
        assert ref.dtype == np.longdouble and ref.shape == (window,)
        direct = np.array([sum(np.longdouble(h[j]) * np.longdouble(w[L - 1 + t - j]) for j in range(L)) for t in range(min(window, 3))])
        assert np.abs(ref[:direct.size] - direct).max() <= 1e-17 * np.abs(h).sum() * np.abs(w).max()
        assert RV.error_scale(h, w, 2048) == 2.0 ** -52 * 11 * np.abs(h).sum() * np.abs(w).max()
        worst = max(worst, RV.numpy_ratio(h, w, 2048))
    assert 0.0 < worst <= 0.5                                        # NumPy's own FFT convolution: a fraction of the scale
    assert RV.numpy_ratio(RV.room(5, 1), np.zeros(20), 2048) == 0.0
    assert RV.bank_lengths(1024) == [1, 2, 1023, 1024, 1025, 2048, 2049, 3089]


# ------------------------------------------------------------------ the command line
def test_check_ir_args_and_read_ir(tmp_path):
    from mrcaudiocodec_amd import cli
    from mrcaudiocodec_amd.store import ir_at_rate
    assert cli.check_ir_args(None, True) is None and cli.check_ir_args(None, False) is None
    assert cli.check_ir_args("room.npy", True) == "room.npy"
    with pytest.raises(ValueError, match="--ir reverberates a decode with an impulse response: it needs -d"):
        cli.check_ir_args("room.npy", False)
    h = RV.room(50, 3)
    npy, wav, stereo = str(tmp_path / "h.npy"), str(tmp_path / "h.wav"), str(tmp_path / "s.wav")
    np.save(npy, h.astype(np.float32))
    assert np.array_equal(cli.read_ir(npy, 16000), h.astype(np.float32).astype(np.float64))
    codes = np.clip(np.rint(h * 20000), -32767, 32767).astype(np.int16)
    with open(wav, "wb") as fp:
        fp.write(cli.wav_bytes(codes[None], 48000))
    x = np.sign(codes) * 2.0 * np.abs(codes.astype(np.float64)) / 65535
    assert np.array_equal(cli.read_ir(wav, 48000), x)
    assert np.array_equal(cli.read_ir(wav, 16000), ir_at_rate(x, 48000, 16000)) and cli.read_ir(wav, 16000).shape == (17,)
    with open(stereo, "wb") as fp:
        fp.write(cli.wav_bytes(np.stack([codes, codes]), 48000))
    with pytest.raises(ValueError, match="--ir: .*a WAV impulse response must have one channel"):
        cli.read_ir(stereo, 48000)
    np.save(npy, np.zeros((2, 2)))
    with pytest.raises(ValueError, match="--ir: impulse response 0 must be 1-D"):
        cli.read_ir(npy, 48000)
    with pytest.raises(ValueError, match="--ir: "):
        cli.read_ir(str(tmp_path / "none.wav"), 48000)


@pytest.mark.parametrize("argv,text", [
    (["in.wav", "out.pac", "--ir", "room.npy"], "--ir reverberates a decode with an impulse response: it needs -d"),
    (["--levels", "a.pac", "--ir", "room.npy"], "--ir reverberates a decode with an impulse response: it needs -d"),
])
def test_cli_refuses_an_ir_without_a_decode(argv, text, capsys):
    from mrcaudiocodec_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2 and text in capsys.readouterr().err
