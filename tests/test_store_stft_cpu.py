"""
The store's STFT (mrc_pac_store_stft_window, PacStore.stft_window, store.hann_window / padded_window / mel_bin_weights /
check_stft) as far as a CPU reaches: the binding against the header, the helpers against restatements in Python floats, the
n_fft rule, every Python-side refusal with a stub in place of the library, and the reference the GPU test measures against.
"""
import math

import numpy as np
import pytest

import chain_kit as kit
import stft_reference as SR
import store_kit

ACCEPTED = (16, 18, 20, 30, 400, 2048)
REFUSED = (14, 22, 401, 2050, 4096)


# ------------------------------------------------------------------ the binding
def test_binding_of_the_stft_calls():
    from mrcaudiocodec_amd import _lib, store
    names = ("mrc_pac_store_stft_window", "mrc_pac_store_stft_ms")
    kit.check_binding(names)
    assert all(hasattr(_lib.lib, n) for n in names)
    name = lambda a: a.split()[-1].lstrip("*")
    args = [name(a) for a in kit.header_args("mrc_pac_store_stft_window")]
    reverb = [name(a) for a in kit.header_args("mrc_pac_store_decode_window_reverb")]
    head = reverb[:reverb.index("ir_of") + 1]
    assert args[:len(head)] == head                      # every argument of the reverb call up to ir_of, in order
    assert args[len(head):] == ["n_fft", "frame_window", "n_frames", "hop", "mode", "n_filters", "bank", "n_channels_out", "format", "out",
                                "stream"]
    assert len(args) == 29 and len(_lib.lib.mrc_pac_store_stft_window.argtypes) == 29
    assert [name(a) for a in kit.header_args("mrc_pac_store_stft_ms")] == ["s", "ms"]
    text = kit.header_text()
    for word, value in (("MRC_STFT_COMPLEX", 0), ("MRC_STFT_POWER", 1), ("MRC_STFT_BANK", 2), ("MRC_MAX_STFT_POINTS", 2048)):
        assert "#define %s %d" % (word, value) in " ".join(text.split()) and getattr(_lib, word) == value
    assert store.MAX_STFT_POINTS == 2048 and store.STFT_OUTPUTS == {"complex": 0, "power": 1, "bank": 2}


# ------------------------------------------------------------------ the helpers
def test_hann_and_padded_windows_follow_their_formulas():
    from mrcaudiocodec_amd.store import hann_window, padded_window
    for n in (1, 2, 16, 400, 401):
        w = hann_window(n)
        assert w.dtype == np.float64 and w.shape == (n,)
        assert np.allclose(w, [0.5 - 0.5 * math.cos(2 * math.pi * k / n) for k in range(n)], rtol=0, atol=1e-15)
        s = hann_window(n, periodic=False)
        want = [1.0] if n == 1 else [0.5 - 0.5 * math.cos(2 * math.pi * k / (n - 1)) for k in range(n)]
        assert np.allclose(s, want, rtol=0, atol=1e-15)
    torch = pytest.importorskip("torch")
    # torch evaluates another expression of the same window: each side rounds its angle (up to 2 pi, so 2 pi 2^-53 = 7e-16
    # absolute) and its result
    assert np.abs(hann_window(400) - torch.hann_window(400, dtype=torch.float64).numpy()).max() <= 2e-15
    w = np.arange(1.0, 401.0)
    p = padded_window(w, 512)                                # torch.stft(win_length=400, n_fft=512): 56 zeros either side
    assert p.shape == (512,) and np.array_equal(p[56:456], w) and not p[:56].any() and not p[456:].any()
    p = padded_window([1.0, 2.0, 3.0], 8)                    # an odd difference: the shorter half in front
    assert p.tolist() == [0, 0, 1, 2, 3, 0, 0, 0]
    assert np.array_equal(padded_window(w, 400), w) and padded_window(w, 400) is not w
    for bad in (dict(win=np.zeros(9), n_fft=8), dict(win=[], n_fft=8), dict(win=np.zeros((2, 2)), n_fft=8), dict(win="hann", n_fft=8)):
        with pytest.raises(ValueError, match="padded_window: "):
            padded_window(**bad)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="hann_window: n must be an int >= 1"):
            hann_window(bad)


def _triangles(n_fft, fs, points, slaney):
    """mel_bin_weights restated in Python floats"""
    rows = []
    for q in range(len(points) - 2):
        a, b, c = (float(v) for v in points[q:q + 3])
        row = []
        for k in range(n_fft // 2 + 1):
            f = k * float(fs) / float(n_fft)
            v = max(0.0, min((f - a) / (b - a), (c - f) / (c - b)))
            row.append(v * (2.0 / (c - a)) if slaney else v)
        rows.append(row)
    return np.array(rows)


@pytest.mark.parametrize("n_fft,fs,n_filters,f_min,f_max,scale", [(400, 16000, 80, 0.0, 8000.0, "htk"), (512, 16000, 40, 20.0, 7600.0, "slaney"),
                                                                 (1024, 48000, 80, 0.0, 24000.0, "htk"), (20, 16000, 5, 0.0, 8000.0, "htk")])
def test_mel_bin_weights_are_the_triangles_on_the_bin_centres(n_fft, fs, n_filters, f_min, f_max, scale):
    from mrcaudiocodec_amd.store import mel_bin_weights, mel_points
    points = mel_points(n_filters, f_min, f_max, scale)
    for norm in (None, "slaney"):
        w = mel_bin_weights(n_fft, fs, points, norm)
        assert w.dtype == np.float64 and w.shape == (n_filters, n_fft // 2 + 1) and w.flags.c_contiguous
        assert np.array_equal(w, _triangles(n_fft, fs, points, norm == "slaney"))
        for row in w:                                        # supports are contiguous runs of positive weights
            nz = np.flatnonzero(row)
            assert nz.size == 0 or np.array_equal(nz, np.arange(nz[0], nz[-1] + 1))
    w = mel_bin_weights(n_fft, fs, points)
    # neighbouring triangles sum to one between the second and the second-last point: a bin there has total weight 1
    f = np.arange(n_fft // 2 + 1) * fs / n_fft
    inner = (f >= points[1]) & (f <= points[-2])
    assert inner.any() and np.abs(w.sum(axis=0)[inner] - 1.0).max() <= 4e-15
    s = mel_bin_weights(n_fft, fs, points, "slaney")
    assert np.array_equal(s, w * (2.0 / (points[2:] - points[:-2]))[:, None])
    # an extra where torchaudio is installed and the case is one it can state (its bins span 0 .. fs // 2 in float32); the
    # restatement in Python floats above is the check
    try:
        import torchaudio
    except ImportError:
        torchaudio = None
    if torchaudio is not None and f_max == fs / 2:
        ta = torchaudio.functional.melscale_fbanks(n_fft // 2 + 1, f_min, f_max, n_filters, fs, None, scale).double().numpy().T
        assert np.abs(ta - w).max() <= 1e-5


def test_a_filter_narrower_than_a_bin_may_be_empty():
    """400 points at 16 kHz: bins 40 Hz apart.  A triangle over 41 .. 79 Hz holds no bin centre and reads zero from every frame
    -- the STFT's own behaviour, and torchaudio's; the line-based filterbank_line_weights averages and is never empty.  One
    that straddles a centre holds that single bin."""
    from mrcaudiocodec_amd.store import mel_bin_weights
    w = mel_bin_weights(400, 16000, [41.0, 60.0, 79.0, 90.0])
    assert w.shape == (2, 201) and not w[0].any()
    assert np.flatnonzero(w[1]).tolist() == [2] and w[1][2] == (90.0 - 80.0) / (90.0 - 79.0)


def test_mel_bin_weights_refusals():
    from mrcaudiocodec_amd.store import mel_bin_weights
    ok = dict(n_fft=400, sample_rate=16000, points_hz=[0.0, 100.0, 200.0])
    for change, text in ((dict(n_fft=401), "n_fft must be an even int"), (dict(n_fft=0), "n_fft must be an even int"),
                         (dict(n_fft=400.0), "n_fft must be an even int"), (dict(sample_rate=0), "sample_rate must be a positive finite"),
                         (dict(sample_rate=float("nan")), "sample_rate must be a positive finite"), (dict(sample_rate="16k"), "sample_rate"),
                         (dict(points_hz=[0.0, 1.0]), "points_hz must hold 3 to"), (dict(points_hz=[0.0, 2.0, 1.0]), "increase strictly"),
                         (dict(norm="area"), 'norm must be None or "slaney"')):
        with pytest.raises(ValueError, match="mel_bin_weights: .*" + text):
            mel_bin_weights(**dict(ok, **change))


# ------------------------------------------------------------------ the n_fft rule, on the Python side (the library's: the GPU test)
def test_the_n_fft_rule():
    from mrcaudiocodec_amd.store import check_stft, stft_points_ok
    for n in ACCEPTED:
        assert stft_points_ok(n) and check_stft(n, 1, 1)[0] == n
    for n in REFUSED + (0, -16, 15, 17, 16.0, True, None, "400"):
        assert not stft_points_ok(n)
        with pytest.raises(ValueError, match="stft_window: n_fft must be an even int in 16..2048 with no prime factor other than 2, 3 and 5"):
            check_stft(n, 1, 1)
    want = [n for n in range(16, 2049, 2) if all(p in (2, 3, 5) for p in _factors(n))]
    assert [n for n in range(0, 2100) if stft_points_ok(n)] == want


def _factors(n):
    out, p = [], 2
    while n > 1:
        while n % p == 0:
            out.append(p)
            n //= p
        p += 1
    return out


def test_check_stft():
    from mrcaudiocodec_amd import _lib
    from mrcaudiocodec_amd.store import check_stft, hann_window
    n_fft, hop, n_frames, window, bank, mode = check_stft(400, 160, 98)
    assert (n_fft, hop, n_frames, bank, mode) == (400, 160, 98, None, _lib.MRC_STFT_POWER) and np.array_equal(window, hann_window(400))
    m = np.ones((3, 201), np.float32)
    out = check_stft(np.int64(400), np.int32(160), 0, np.arange(400, dtype=np.float32), m, "bank")
    assert out[3].dtype == np.float64 and out[3].flags.c_contiguous and out[4].dtype == np.float64 and out[4].shape == (3, 201)
    assert out[5] == _lib.MRC_STFT_BANK and check_stft(16, 1, 1, output="complex")[5] == _lib.MRC_STFT_COMPLEX
    assert check_stft(16, 1 << 40, 1)[1] == 1 << 40 and check_stft(16, 1, (1 << 40) - 15)[2] == (1 << 40) - 15
    ok = dict(n_fft=400, hop=160, n_frames=4)
    for change, text in (
            (dict(hop=0), "hop must be an int >= 1"), (dict(hop=1.0), "hop must be an int >= 1"), (dict(hop=True), "hop must be an int >= 1"),
            (dict(n_frames=-1), "n_frames must be an int >= 0"), (dict(n_frames=2.5), "n_frames must be an int >= 0"),
            (dict(n_frames=3, hop=1 << 40), r"must not exceed 2\^40"), (dict(n_frames=(1 << 40) - 398, hop=1), r"must not exceed 2\^40"),
            (dict(output="mel"), 'output must be "power", "complex" or "bank"'), (dict(output=1), "output must be"),
            (dict(frame_window=np.ones(399)), r"frame_window must hold n_fft = 400 taps .* got shape \(399,\)"),
            (dict(frame_window=np.ones((1, 400))), "frame_window must hold n_fft = 400 taps"), (dict(frame_window="hann"), "frame_window must be 400 float taps"),
            (dict(frame_window=np.where(np.arange(400) == 7, np.inf, 1.0)), "frame_window must be finite, tap 7 is not"),
            (dict(bank=np.ones((2, 201))), 'bank goes with output="bank"'), (dict(output="bank"), 'output="bank" needs a bank'),
            (dict(output="bank", bank=np.ones((2, 200))), r"bank must be \[1..256 filters\]\[n_fft // 2 \+ 1 = 201 bins\], got shape \(2, 200\)"),
            (dict(output="bank", bank=np.ones(201)), "bank must be"), (dict(output="bank", bank=np.ones((0, 201))), "bank must be"),
            (dict(output="bank", bank=np.ones((257, 201))), "bank must be"), (dict(output="bank", bank=[["a"] * 201]), "bank must be a float matrix"),
            (dict(output="bank", bank=np.full((2, 201), np.nan)), "bank must be finite")):
        with pytest.raises(ValueError, match="stft_window: .*" + text):
            check_stft(**dict(ok, **change))


# ------------------------------------------------------------------ PacStore.stft_window's refusals, before any library call
def _husk(monkeypatch):
    return store_kit.husk(monkeypatch, n_irs=3)


def test_argument_errors_are_value_errors_before_any_library_call(monkeypatch):
    torch = pytest.importorskip("torch")
    s = _husk(monkeypatch)
    ok = dict(files=[0, 1], starts=[0, 5], n_frames=3, hop=4, n_fft=16)
    cases = [
        # the STFT's own
        (dict(n_fft=22), "n_fft must be an even int in 16..2048"), (dict(n_fft=4096), "n_fft must be an even int"), (dict(hop=0), "hop must be an int >= 1"),
        (dict(n_frames=-1), "n_frames must be an int >= 0"), (dict(output="db"), "output must be"), (dict(frame_window=np.ones(15)), "frame_window must hold n_fft = 16 taps"),
        (dict(frame_window=[float("nan")] * 16), "frame_window must be finite, tap 0"), (dict(bank=np.ones((2, 9))), 'bank goes with output="bank"'),
        (dict(output="bank"), 'output="bank" needs a bank'), (dict(output="bank", bank=np.ones((2, 8))), "bank must be"),
        (dict(center=1), "center must be True or False"), (dict(center="yes"), "center must be True or False"),
        (dict(dtype=torch.int16), "dtype must be torch.float32 or torch.float64"), (dict(dtype=torch.complex64), "dtype must be torch.float32 or torch.float64, got"),
        (dict(output="complex", dtype=torch.float16), r"dtype must be torch.float32 or torch.float64 \(or complex64 / complex128\)"),
        (dict(channels=3), "channels must be None, 1 or 2"), (dict(out=np.zeros((2, 2, 9, 3), np.float32)), "out must be a contiguous torch.float32 tensor of shape"),
        (dict(out=torch.zeros((2, 2, 9, 4))), r"out must be a contiguous torch.float32 tensor of shape \(2, 2, 9, 3\)"),
        (dict(output="complex", out=torch.zeros((2, 2, 9, 3))), "out must be a contiguous torch.complex64 tensor"),
        # the rows', as decode_window_sum's, under this call's name
        (dict(starts=[0]), "one start per file index"), (dict(item_offsets=[0, 1, 2]), "item_offsets goes with gains"),
        (dict(gains=[1.0]), "files, starts and gains must have one shape"), (dict(gains=[1.0, 0.5]), r"must be \[n\]\[K\], or 1-D with item_offsets"),
        (dict(gains=[1.0, float("inf")], item_offsets=[0, 2]), "gains must be finite"), (dict(gains=[1.0, 0.5], item_offsets=[1, 2]), "item_offsets must be"),
        (dict(rate_divisor=3), "rate_divisor"), (dict(mix="side"), "mix"), (dict(mix="mid", channels=2), "mix"), (dict(resample=(0, 1)), "resample"),
        (dict(band_edges_hz=[0, 100]), "band_edges_hz"), (dict(band_gains=[[1.0]]), "band_gains"), (dict(speed_index=[0, 0]), "speed_factors and speed_index go together"),
        (dict(speed_factors=[(1, 1)], speed_index=[0, 1]), "speed_index"), (dict(ir_index=[0, 3]), r"ir_index must be -1 or lie in 0\.\.2"),
        (dict(ir_index=[0]), "ir_index must have shape"),
    ]
    for change, text in cases:
        with pytest.raises(ValueError, match="stft_window: .*" + text):
            s.stft_window(**dict(ok, **change))


# ------------------------------------------------------------------ the GPU test's reference and unit
def test_the_reference_and_the_unit():
    rng = np.random.default_rng(0)
    worst = 0.0
    for n_fft in (16, 20, 30, 400, 512):
        gx = rng.standard_normal((3, n_fft))
        gx[1] = np.cos(2 * np.pi * 3 * np.arange(n_fft) / n_fft)          # a pure tone on a bin centre
        gx[2, 1:] = 0.0                                                   # an impulse: a flat spectrum
        re, im = SR.dft(gx)
        assert re.dtype == np.longdouble and re.shape == (3, n_fft // 2 + 1) == im.shape
        k = n_fft // 2 - 1                                                # ... against the sum said directly
        direct = sum(np.longdouble(gx[0][n]) * np.exp(-2j * np.pi * ((k * n) % n_fft) / n_fft) for n in range(n_fft))
        assert abs(complex(re[0][k], im[0][k]) - direct) <= 1e-13 * np.abs(gx[0]).sum()
        assert np.abs(re[2] - gx[2, 0]).max() == 0 and np.abs(im[2]).max() == 0
        # (the tone's own samples are rounded to float64: up to 2^-53 each leaks into every bin)
        assert abs(re[1][3] - n_fft / 2) <= 2.0 ** -52 * n_fft and np.abs(np.delete(re[1], 3)).max() <= 2.0 ** -52 * n_fft
        u = SR.unit(gx)
        assert np.array_equal(u, 2.0 ** -52 * np.log2(n_fft) * np.sqrt((gx * gx).sum(axis=1)))
        worst = max(worst, SR.numpy_ratio(gx))
        # a float32 table is far outside any multiple of the unit that a float64 transform needs
        r32, i32 = SR.dft(gx, np.float32)
        assert SR.ratio(r32.astype(np.float64), i32.astype(np.float64), re, im, u) > 1e4
    assert 0.0 < worst <= 2.0                                             # NumPy's own transform: of the order of the unit
    frames = SR.frames_of(np.arange(20.0)[None], 8, 5, 3)
    assert frames.shape == (1, 3, 8) and frames[0, 2].tolist() == list(range(10, 18))
    assert SR.ratio(np.zeros((1, 5)), np.zeros((1, 5)), np.zeros((1, 5), np.longdouble), np.zeros((1, 5), np.longdouble), np.zeros(1)) == 0.0
    assert SR.ratio(np.ones((1, 5)), np.zeros((1, 5)), np.zeros((1, 5), np.longdouble), np.zeros((1, 5), np.longdouble), np.zeros(1)) == np.inf
