"""
CPU tests of the store's filter-bank energies (mrc_filterbank_line_weights, store.mel_points, PacStore.filterbank_window's
argument checks, cli --filterbank-energies' argument checks, tests/filterbank_restatement.py): the host rule against the
restatement to the bit, its properties and refusals; the mel points; the Python and command-line refusals before any library
call; what the estimate resolves (oracle transforms only, an analytic reference).  No GPU.
"""
import numpy as np
import pytest

import bands_restatement as BR
import chain_kit as kit
import filterbank_restatement as FR
import levels_restatement as LR
import settings_kit as SK

SETTINGS = tuple(SK.SETTINGS) + ("default",)
SETS = ("mel", "slaney", "one", "narrow", "full")


def _cfg(sid):
    from mrcaudiocodec_amd import pacfile
    return pacfile.make_config() if sid == "default" else SK.config(sid)


def _shapes(cfg):
    L, S = cfg.n_mdct_lines, cfg.n_short
    return ((L, L), (L, S), (S, L), (S, S))


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.int64), b.view(np.int64))


# ------------------------------------------------------------------ the host rule
@pytest.mark.parametrize("sid", SETTINGS)
def test_line_weights_equal_the_restatement_to_the_bit_and_keep_their_properties(sid):
    from mrcaudiocodec_amd import _lib, store
    cfg = _cfg(sid)
    fs = cfg.sample_rate
    worst_unity = 0.0
    for name, (points, _) in FR.filter_sets(fs).items():
        assert name in SETS
        n = len(points) - 2
        for a, b in _shapes(cfg):
            half = (a + b) // 2
            d = (float(fs) / half) / 2.
            for norm in (None, "slaney"):
                lo, hi, rows = store.filterbank_line_weights(fs, a, b, points, norm)
                wlo, whi, wrows = FR.line_weights(fs, a, b, points, norm)
                assert lo.dtype == hi.dtype == np.int32 and np.array_equal(lo, wlo) and np.array_equal(hi, whi), (sid, name, a, b)
                assert len(rows) == n and all(_same(r, w) for r, w in zip(rows, wrows)), (sid, name, a, b, norm)
                # the sizes-only call agrees with the full call
                l2, h2, count = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(1, np.int64)
                assert _lib.lib.mrc_filterbank_line_weights(float(fs), a, b, n, np.ascontiguousarray(points).ctypes.data,
                                                            store.FILTER_NORMS[norm], l2.ctypes.data, h2.ctypes.data, 0, None,
                                                            count.ctypes.data) == 0
                assert np.array_equal(l2, lo) and np.array_equal(h2, hi) and int(count[0]) == sum(len(r) for r in rows)
                # properties
                assert np.all(hi >= lo) and np.all(hi <= half) and all(len(r) == h - l for r, l, h in zip(rows, lo, hi))
                assert all(np.all(r >= 0) for r in rows)
                for q in range(n):                                   # no filter below the last line's upper edge is empty
                    if points[q] < half * d:
                        assert len(rows[q]) and rows[q].max() > 0, (sid, name, a, b, q)
                assert int(count[0]) <= 2 * half + 2 * n
                if norm is None and n > 1:                           # a line inside [point[1], point[n]]: its weights add up to 1
                    total = np.zeros(half)
                    for q in range(n):
                        total[lo[q]:hi[q]] += rows[q]
                    e = np.arange(half + 1) * d
                    inside = (e[:-1] >= points[1]) & (e[1:] <= points[n])
                    if inside.any():
                        worst_unity = max(worst_unity, float(np.abs(total[inside] - 1.0).max()))
                        assert np.all(np.abs(total[inside] - 1.0) <= 1e-12), (sid, name, a, b)
                    assert np.all(total <= 1.0 + 1e-12)
    print("%s: the weights of a line inside the bank add up to 1 within %.3g" % (sid, worst_unity))


def test_line_weight_refusals():
    from mrcaudiocodec_amd import MrcError, _lib, store
    ok = [0.0, 1000.0, 24000.0]
    lo, hi, rows = store.filterbank_line_weights(48000, 1024, 1024, ok)
    assert lo.tolist() == [0] and hi.tolist() == [1024] and len(rows[0]) == 1024
    for points, word in (([0.0, 1.0], "n_filters 0"), ([0.0], "n_filters -1"), (np.arange(259.0), "n_filters 257"),
                         ([0.0, np.inf, 5.0], "point_hz[1] is not finite"), ([np.nan, 5.0, 6.0], "point_hz[0] is not finite"),
                         ([-1.0, 5.0, 6.0], "point_hz[0] < 0"), ([0.0, 5.0, 5.0], "not strictly increasing at [2]"),
                         ([0.0, 0.0, 5.0], "not strictly increasing at [1]"), ([0.0, 7.0, 5.0], "not strictly increasing at [2]")):
        with pytest.raises(MrcError, match=r"mrc_filterbank_line_weights: .*%s" % word.replace("[", r"\[").replace("]", r"\]")) as e:
            store.filterbank_line_weights(48000, 1024, 1024, points)
        assert e.value.code == _lib.MRC_ERR_INVALID
    with pytest.raises(ValueError, match="norm must be None"):
        store.filterbank_line_weights(48000, 1024, 1024, ok, "htk")

    def raw(a=1024, b=1024, norm=0, cap=1024, weight=True, fs=48000.0):
        p = np.array(ok)
        l, h, w, n = np.zeros(1, np.int32), np.zeros(1, np.int32), np.full(1025, 77.0), np.zeros(1, np.int64)
        rc = _lib.lib.mrc_filterbank_line_weights(fs, a, b, 1, p.ctypes.data, norm, l.ctypes.data, h.ctypes.data, cap,
                                                  w.ctypes.data if weight else None, n.ctypes.data)
        return rc, _lib.lib.mrc_last_error(None).decode(), w, int(n[0])

    for norm in (2, -1):
        rc, text, w, _ = raw(norm=norm)
        assert rc == _lib.MRC_ERR_INVALID and "mrc_filterbank_line_weights: norm %d" % norm in text and np.all(w == 77.0)
    rc, text, w, _ = raw(fs=0.0)
    assert rc == _lib.MRC_ERR_INVALID and "sample_rate" in text
    for a, b in ((0, 0), (-4, 8), (1024, 3)):
        assert _lib.lib.mrc_synthesis_shape(a, b, 1) == _lib.MRC_ERR_INVALID
        why = _lib.lib.mrc_last_error(None).decode().split("mrc_synthesis_shape: ")[1]
        rc, text, _, _ = raw(a=a, b=b)
        assert rc == _lib.MRC_ERR_INVALID and "mrc_filterbank_line_weights: " + why in text
    rc, text, w, _ = raw(cap=1023)
    assert rc == _lib.MRC_ERR_INVALID and "weight_cap 1023" in text and "1024" in text and np.all(w == 77.0)
    rc, _, w, n = raw(cap=0, weight=False)                           # sizes only: the cap is not looked at
    assert rc == 0 and n == 1024 and np.all(w == 77.0)
    rc, _, w, n = raw()
    assert rc == 0 and n == 1024 and w[1024] == 77.0 and np.all(w[:1024] != 77.0)
    full = np.arange(258.0)
    assert len(store.filterbank_line_weights(48000, 1024, 1024, full)[2]) == 256


def test_binding_of_the_filterbank_calls():
    from mrcaudiocodec_amd import _lib
    kit.check_binding(("mrc_filterbank_line_weights", "mrc_pac_store_filterbank_window"))
    args = kit.header_args("mrc_pac_store_filterbank_window")
    assert args[:3] == ["mrc_pac_store* s", "int mix", "int64_t n_items"] and args[-1] == "void* stream" and len(args) == 14
    assert args[7:10] == ["int n_filters", "const double* point_hz", "int norm"]
    args = kit.header_args("mrc_filterbank_line_weights")
    assert len(args) == 11 and args[0] == "double sample_rate" and args[-1] == "int64_t* n_weights"
    text = kit.header_text()
    assert int(text.split("#define MRC_FILTER_NORM_NONE")[1].split()[0]) == _lib.MRC_FILTER_NORM_NONE == 0
    assert int(text.split("#define MRC_FILTER_NORM_SLANEY")[1].split()[0]) == _lib.MRC_FILTER_NORM_SLANEY == 1


# ------------------------------------------------------------------ the mel points
def test_mel_points():
    from mrcaudiocodec_amd import store
    for n, f_min, f_max, scale in ((80, 0, 24000, "htk"), (80, 20, 8000, "htk"), (128, 0.0, 24000.0, "htk"), (40, 50, 20000, "htk"),
                                   (40, 50, 19200.0, "slaney"), (1, 0, 1, "slaney"), (256, 0, 22050, "slaney"), (3, 900, 1100, "slaney")):
        p = store.mel_points(n, f_min, f_max, scale)
        assert p.dtype == np.float64 and p.shape == (n + 2,) and np.all(np.diff(p) > 0)
        assert p[0] == float(f_min) and p[-1] == float(f_max)          # the ends exactly
        m = np.array([FR.hz_to_mel(float(v), scale) for v in p])         # equally spaced in the restated mel map
        want = np.linspace(m[0], m[-1], n + 2)
        assert np.all(np.abs(m - want) <= 1e-9 * max(abs(want[-1]), 1.0)), (n, scale)
        back = store.mel_to_hz(store.hz_to_mel(p, scale), scale)       # the map inverts itself
        assert np.all(np.abs(back - p) <= 1e-9 * np.maximum(p, 1.0))
        assert np.array_equal(store.check_filter_points(p), p)
    htk, slaney = store.mel_points(30, 0, 1000, "htk"), store.mel_points(30, 0, 1000, "slaney")
    assert np.all(np.diff(htk) > 0) and np.all(np.diff(slaney) > 0)    # below 1 kHz: both increase, nothing else in common
    assert store.mel_points(80, 0, 24000).tolist() == store.mel_points(80, 0, 24000, "htk").tolist()
    for kw in (dict(n_filters=0), dict(n_filters=257), dict(n_filters=2.0), dict(n_filters=True), dict(f_min=-1), dict(f_max=0),
               dict(f_min=100, f_max=100), dict(f_min=200, f_max=100), dict(f_max=np.inf), dict(f_min=np.nan), dict(f_max="8k"),
               dict(scale="bark"), dict(scale=None), dict(f_min=1.0, f_max=np.nextafter(1.0, 2.0), n_filters=5)):
        with pytest.raises(ValueError, match="mel_points: "):
            store.mel_points(**dict(dict(n_filters=10, f_min=0, f_max=8000, scale="htk"), **kw))


# ------------------------------------------------------------------ Python-side refusals
from store_kit import husk as _husk


def test_filterbank_window_refuses_bad_arguments_before_any_library_call(monkeypatch):
    torch = pytest.importorskip("torch")
    s = _husk(monkeypatch)
    ok = dict(files=[0], starts=[0], n_frames=4, hop=512, points_hz=[0.0, 1000.0, 24000.0])

    def refused(match, **kw):
        with pytest.raises(ValueError, match="filterbank_window: .*" + match):
            s.filterbank_window(**dict(ok, **kw))

    for bad in ("side", "Mid", "", 0, True, "each"):
        refused("mix must be None", mix=bad)
    refused("gives one channel", mix="mid", channels=2)
    refused("one start per file index", starts=[0, 1])
    for bad in (-1, 2.0, True, None, "4"):
        refused("n_frames must be an int >= 0", n_frames=bad)
    for bad in (0, -3, 512.0, False, None):
        refused("hop must be an int >= 1", hop=bad)
    refused("2\\^62", n_frames=1 << 31, hop=1 << 32)
    for bad in ([0.0, 1.0], [], np.arange(259.0), "abc", None):
        refused("points_hz must", points_hz=bad)
    refused("finite", points_hz=[0.0, 5.0, np.inf])
    refused("increase strictly", points_hz=[0.0, 5.0, 5.0])
    refused("at or above 0", points_hz=[-1.0, 5.0, 6.0])
    for bad in ("htk", "Slaney", 1, True, 0):
        refused("norm must be None or \"slaney\"", norm=bad)
    for bad in (torch.int16, torch.float16, np.float32):
        refused("dtype must be torch.float32 or torch.float64", dtype=bad)
    for bad in (0, 3, True, 1.0):
        refused("channels must be None, 1 or 2", channels=bad)
    for bad in ([2], [-1]):
        refused("indices into the store", files=bad)
    refused("stereo file in a one-channel call", channels=1)
    refused("out must be a contiguous", out=np.zeros((1, 2, 1, 4), np.float32), dtype=torch.float32)
    refused("out must be a contiguous", out=torch.zeros((1, 2, 1, 5)))
    refused("out must be a contiguous", out=torch.zeros((1, 2, 1, 4)), dtype=torch.float64)


FB = ["--filterbank-energies", "a.pac", "o.npy"]


@pytest.mark.parametrize("argv,text", [
    (FB + ["--mel", "80"], "--hop"),
    (FB + ["--mel", "80", "--hop", "0"], "--hop"),
    (["--filterbank-energies", "a.pac", "--hop", "480", "--mel", "80"], "src, dst"),
    (FB + ["--hop", "480"], "exactly one of --mel N and --filter-points"),
    (FB + ["--hop", "480", "--mel", "80", "--filter-points", "0,100,200"], "exactly one of --mel N and --filter-points"),
    (FB + ["--hop", "480", "--mel", "0"], "--mel"),
    (FB + ["--hop", "480", "--mel", "257"], "--mel"),
    (FB + ["--hop", "480", "--mel", "80", "--mel-scale", "bark"], "--mel-scale"),
    (FB + ["--hop", "480", "--mel", "80", "--f-min", "-5"], "--f-min"),
    (FB + ["--hop", "480", "--mel", "80", "--f-min", "500", "--f-max", "400"], "f_min < f_max"),
    (FB + ["--hop", "480", "--mel", "80", "--f-max", "inf"], "--f-max"),
    (FB + ["--hop", "480", "--mel", "80", "--filter-norm", "htk"], "--filter-norm"),
    (FB + ["--hop", "480", "--filter-points", "0,x,5"], "--filter-points"),
    (FB + ["--hop", "480", "--filter-points", "0,500,400"], "--filter-points"),
    (FB + ["--hop", "480", "--filter-points", "0,100"], "--filter-points"),
    (FB + ["--hop", "480", "--filter-points", "0,100,200", "--f-min", "3"], "--f-min goes with --mel"),
    (FB + ["--hop", "480", "--filter-points", "0,100,200", "--mel-scale", "htk"], "--mel-scale goes with --mel"),
    (FB + ["--hop", "480", "--mel", "80", "-d"], "does not go with -d"),
    (FB + ["--hop", "480", "--mel", "80", "--bits-per-sample", "2"], "does not go with --bits-per-sample"),
    (FB + ["--hop", "480", "--mel", "80", "--start", "3"], "does not go with --start"),
    (FB + ["--hop", "480", "--mel", "80", "--rate-divisor", "2"], "does not go with --rate-divisor"),
    (FB + ["--hop", "480", "--mel", "80", "--levels", "b.pac"], "does not go with --levels"),
    (FB + ["--hop", "480", "--mel", "80", "--band-energies"], "does not go with --band-energies"),
    (FB + ["--hop", "480", "--mel", "80", "--band-edges", "0,100"], "does not go with --band-edges"),
    (FB + ["--hop", "480", "--mel", "80", "--mix", "side"], "--mix"),
    (["--band-energies", "a.pac", "o.npy", "--hop", "512", "--mel", "80"], "--mel belongs to --filterbank-energies"),
    (["-d", "in.pac", "out.wav", "--filter-points", "0,100,200"], "--filter-points belongs to --filterbank-energies"),
    (["in.wav", "out.pac", "--filter-norm", "slaney"], "--filter-norm belongs to --filterbank-energies"),
])
def test_cli_refuses_filterbank_arguments_that_make_no_sense(argv, text, capsys):
    """before a file is read: a.pac does not exist"""
    from mrcaudiocodec_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2 and text in capsys.readouterr().err


def test_check_filterbank_energies_args():
    from mrcaudiocodec_amd import cli
    none = (None,) * 6
    assert cli.check_filterbank_energies_args(False, None, *none, {}) is None
    hop, bank = cli.check_filterbank_energies_args(True, 480, 80, None, None, None, None, None, {})
    assert hop == 480 and bank == dict(points=None, mel=(80, 0.0, None, "htk"), norm=None)
    hop, bank = cli.check_filterbank_energies_args(True, 100, 40, 50.0, 8000.0, "slaney", None, "slaney", {})
    assert bank == dict(points=None, mel=(40, 50.0, 8000.0, "slaney"), norm="slaney")
    hop, bank = cli.check_filterbank_energies_args(True, 100, None, None, None, None, "0,50.5,2e3", None, {})
    assert bank["points"].tolist() == [0.0, 50.5, 2000.0] and bank["mel"] is None
    for flag in cli.FILTERBANK_ENERGIES_REFUSES:
        with pytest.raises(ValueError, match="does not go with %s" % flag):
            cli.check_filterbank_energies_args(True, 480, 80, None, None, None, None, None, {flag: True})
    assert set(cli.BAND_ENERGIES_REFUSES) < set(cli.FILTERBANK_ENERGIES_REFUSES) and "src" not in cli.FILTERBANK_ENERGIES_REFUSES


# ------------------------------------------------------------------ what the estimate resolves
TONES = ((0.25, 1000.0), (0.075, 5200.0))
PAIR_BOUND_DB = 2 * 1.909                                            # twice the largest pair-sum error measured (docstring below)


def _tone_probe(seed):
    """test_store_bands_cpu._tone_probe's construction, restated: oracle transforms only, no quantiser: L = 1024, S = 128, 40
    hops of which 20 % are short at random; a 0.25 tone at 1 kHz and a 0.075 tone at 5.2 kHz over 0.01 white noise; frames of
    4096 samples, the 80 mel filters over 0 - 24 kHz.  -> (est [80][10], true frame totals [10], the points, hop)"""
    L, S, hops, fs, hop = 1024, 128, 40, 48000, 4096
    rng = np.random.default_rng(seed)
    short = rng.random(hops) < 0.2
    n = hops * L
    t = np.arange(n)
    x = sum(A * np.sin(2 * np.pi * f / fs * t) for A, f in TONES) + 0.01 * rng.standard_normal(n)
    seq = LR.block_sequence(hops + 1, list(short) + [False], L, S)
    lines = LR.analyse(x, seq, L)
    points, norm = FR.filter_sets(fs)["mel"]
    rows = {}
    F = []
    for (p, a, b), X in zip(seq, lines):
        if (a, b) not in rows:
            rows[(a, b)] = FR.line_weights(fs, a, b, points, norm)
        F.append(FR.filter_sums(X, rows[(a, b)]))
    est, _ = BR.frames(seq, np.array(F), L, 0, n // hop, hop)
    true = (x * x).reshape(-1, hop).sum(axis=1)
    return est, true, points, hop


def test_tone_filters_read_the_tones_energy():
    """The reference is analytic: a tone of amplitude A at f puts A^2 / 2 * hop * w_q(f) into filter q, w_q the triangle's value
    at f, and the two filters that hold f have w adding up to 1.  Held: the SUM of those two filters within 2 x 1.909 = 3.82 dB
    of A^2 / 2 * hop on every frame of seeds 0-4 (twice the largest error measured: the band test's margin for seeds not tried).
    Measured, seeds 0-4, the largest error over the frames:
        tone       pair sum    single filter (against A^2 / 2 hop w_q(f))
        1 kHz      1.909 dB    3.112 dB    (points 75.9 Hz apart: 0.4 of a short block's line, 187.5 Hz)
        5.2 kHz    0.413 dB    0.569 dB    (points 260.1 Hz apart)
    and a frame's total over the un-normalised bank is 0.921 to 1.026 of the true sum of squares.  Nothing is asserted on
    single filters or on the other filters: they carry the window's leakage and the short blocks' line spacing."""
    worst, totals = 0.0, []
    for seed in range(5):
        est, true, points, hop = _tone_probe(seed)
        for A, f in TONES:
            i = int(np.searchsorted(points, f, side="right")) - 1    # f in [points[i], points[i + 1]): filters i - 1 and i
            assert 1 <= i <= len(points) - 3
            w_fall = (points[i + 1] - f) / (points[i + 1] - points[i])
            w_rise = (f - points[i]) / (points[i + 1] - points[i])
            full = A * A / 2 * hop
            pair = np.abs(10 * np.log10((est[i - 1] + est[i]) / full))
            single = max(np.abs(10 * np.log10(est[i - 1] / (full * w_fall))).max(), np.abs(10 * np.log10(est[i] / (full * w_rise))).max())
            print("seed %d, %g Hz in filters %d and %d (%.1f Hz wide): pair sum within %.3f dB, single filters within %.3f dB, %d frames"
                  % (seed, f, i - 1, i, points[i + 1] - points[i], pair.max(), single, pair.size))
            worst = max(worst, float(pair.max()))
        ratio = est.sum(axis=0) / true
        totals += [float(ratio.min()), float(ratio.max())]
        print("seed %d: a frame's total over the bank is %.3f to %.3f of the true sum of squares" % (seed, ratio.min(), ratio.max()))
    print("largest pair-sum error %.3f dB; frame totals %.3f to %.3f of the true totals" % (worst, min(totals), max(totals)))
    assert worst <= PAIR_BOUND_DB
