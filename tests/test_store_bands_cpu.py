"""
CPU tests of the store's band energies (mrc_band_line_ranges, PacStore.band_energy_window's argument checks, cli
--band-energies' argument checks, tests/bands_restatement.py): the host rule against NumPy and against mrc_band_table, its
refusals; the Python and command-line refusals before any library call; what the estimate resolves (oracle transforms
only); the full-coverage identity of the restatement against the block energies and the decoded signal.  No GPU.
"""
import numpy as np
import pytest

import bands_restatement as BR
import chain_kit as kit
import levels_restatement as LR
import reduced_restatement as RR
import settings_kit as SK

SETTINGS = tuple(SK.SETTINGS) + ("default",)


def _cfg(sid):
    from mrcaudiocodec_amd import pacfile
    return pacfile.make_config() if sid == "default" else SK.config(sid)


def _shapes(cfg):
    L, S = cfg.n_mdct_lines, cfg.n_short
    return ((L, L), (L, S), (S, L), (S, S))


# ------------------------------------------------------------------ the host rule
@pytest.mark.parametrize("sid", SETTINGS)
def test_line_ranges_equal_the_numpy_rule_and_the_codecs_band_table(sid):
    from mrcaudiocodec_amd import pacfile, store
    cfg = _cfg(sid)
    fs = cfg.sample_rate
    edges = store.critical_band_edges(fs)
    assert np.array_equal(edges, BR.critical_edges(fs)) and edges[0] == 0.0 and edges[-1] == fs / 2.0
    rng = np.random.default_rng(11)
    for a, b in _shapes(cfg):
        half = (a + b) // 2
        lo = store.band_line_ranges(fs, a, b, edges)
        assert lo.dtype == np.int32 and np.array_equal(lo, BR.line_ranges(fs, a, b, edges))
        assert lo[0] == 0 and lo[-1] == half and np.all(np.diff(lo) >= 0)       # every line centre lies in [0, fs / 2)
        if a == b == cfg.n_mdct_lines:                              # the long block's table uses these limits
            table = pacfile.band_table(cfg, a, b)
            assert len(table) == len(edges) - 1 == 25 and np.array_equal(np.diff(lo), table)
        # random edges, some above Nyquist, some closer together than the lines
        for n in (1, 7, 256):
            e = np.sort(rng.uniform(0.0, 0.7 * fs, n + 1))
            if np.any(np.diff(e) <= 0):
                continue
            got = store.band_line_ranges(fs, a, b, e)
            assert np.array_equal(got, BR.line_ranges(fs, a, b, e)), (sid, a, b, n)
            assert got[-1] <= half
        # an edge exactly on a line centre: the line is NOT below it (psychoac.py:99 compares with <)
        k = half // 3
        fk = (k + 0.5) * ((float(fs) / half) / 2.)
        assert store.band_line_ranges(fs, a, b, [fk, np.nextafter(fk, np.inf)]).tolist() == [k, k + 1]
    # narrow bands read no line of a short block
    S = cfg.n_short
    narrow = BR.narrow_edges(fs)
    assert np.diff(narrow).min() < (fs / 2.0) / S and np.any(np.diff(store.band_line_ranges(fs, S, S, narrow)) == 0)


def test_line_range_refusals():
    from mrcaudiocodec_amd import MrcError, _lib, store
    ok = [0.0, 1000.0, 24000.0]
    assert store.band_line_ranges(48000, 1024, 1024, ok).tolist() == [0, 43, 1024]
    for edges, word in (([0.0], "n_bands 0"), (np.arange(258.0), "n_bands 257"), ([0.0, np.inf], "edge_hz[1] is not finite"),
                        ([np.nan, 5.0], "edge_hz[0] is not finite"), ([-1.0, 5.0], "edge_hz[0] < 0"),
                        ([0.0, 5.0, 5.0], "not strictly increasing at [2]"), ([0.0, 7.0, 5.0], "not strictly increasing at [2]")):
        with pytest.raises(MrcError, match=r"mrc_band_line_ranges: .*%s" % word.replace("[", r"\[").replace("]", r"\]")) as e:
            store.band_line_ranges(48000, 1024, 1024, edges)
        assert e.value.code == _lib.MRC_ERR_INVALID
    for a, b in ((0, 0), (-4, 8), (1024, 3)):
        assert _lib.lib.mrc_synthesis_shape(a, b, 1) == _lib.MRC_ERR_INVALID
        why = _lib.lib.mrc_last_error(None).decode().split("mrc_synthesis_shape: ")[1]
        with pytest.raises(MrcError) as e:
            store.band_line_ranges(48000, a, b, ok)
        assert e.value.code == _lib.MRC_ERR_INVALID and "mrc_band_line_ranges: " + why in str(e.value)
    assert np.array_equal(store.band_line_ranges(48000, 1024, 1024, np.arange(257.0)), BR.line_ranges(48000, 1024, 1024, np.arange(257.0)))


def test_binding_of_the_band_calls():
    from mrcaudiocodec_amd import store
    kit.check_binding(("mrc_band_line_ranges", "mrc_pac_store_band_energy_window"))
    args = kit.header_args("mrc_pac_store_band_energy_window")
    assert args[:3] == ["mrc_pac_store* s", "int mix", "int64_t n_items"] and args[-1] == "void* stream" and len(args) == 13
    text = kit.header_text()
    assert int(text.split("#define MRC_MAX_STORE_BANDS")[1].split()[0]) == store.MAX_BANDS == 256


# ------------------------------------------------------------------ Python-side refusals
from store_kit import husk as _husk


def test_band_energy_window_refuses_bad_arguments_before_any_library_call(monkeypatch):
    torch = pytest.importorskip("torch")
    s = _husk(monkeypatch)
    ok = dict(files=[0], starts=[0], n_frames=4, hop=512, band_edges_hz=[0.0, 24000.0])

    def refused(match, **kw):
        with pytest.raises(ValueError, match=match):
            s.band_energy_window(**dict(ok, **kw))

    for bad in ("side", "Mid", "", 0, True, "each"):
        refused("mix must be None", mix=bad)
    refused("gives one channel", mix="mid", channels=2)
    refused("one start per file index", starts=[0, 1])
    for bad in (-1, 2.0, True, None, "4"):
        refused("n_frames must be an int >= 0", n_frames=bad)
    for bad in (0, -3, 512.0, False, None):
        refused("hop must be an int >= 1", hop=bad)
    refused("2\\^62", n_frames=1 << 31, hop=1 << 32)
    for bad in ([0.0], [], np.arange(258.0), "abc", None):
        refused("band_edges_hz must", band_edges_hz=bad)
    refused("finite", band_edges_hz=[0.0, np.inf])
    refused("increase strictly", band_edges_hz=[0.0, 5.0, 5.0])
    refused("at or above 0", band_edges_hz=[-1.0, 5.0])
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


@pytest.mark.parametrize("argv,text", [
    (["--band-energies", "a.pac", "o.npy"], "--hop"),
    (["--band-energies", "a.pac", "o.npy", "--hop", "0"], "--hop"),
    (["--band-energies", "a.pac", "--hop", "512"], "src, dst"),
    (["--band-energies", "a.pac", "o.npy", "--hop", "512", "-d"], "does not go with -d"),
    (["--band-energies", "a.pac", "o.npy", "--hop", "512", "--bits-per-sample", "2"], "does not go with --bits-per-sample"),
    (["--band-energies", "a.pac", "o.npy", "--hop", "512", "--start", "3"], "does not go with --start"),
    (["--band-energies", "a.pac", "o.npy", "--hop", "512", "--rate-divisor", "2"], "does not go with --rate-divisor"),
    (["--band-energies", "a.pac", "o.npy", "--hop", "512", "--levels", "b.pac"], "does not go with --levels"),
    (["--band-energies", "a.pac", "o.npy", "--hop", "512", "--mix", "side"], "--mix"),
    (["--band-energies", "a.pac", "o.npy", "--hop", "512", "--band-edges", "0,x"], "--band-edges"),
    (["--band-energies", "a.pac", "o.npy", "--hop", "512", "--band-edges", "0,500,400"], "--band-edges"),
    (["--band-energies", "a.pac", "o.npy", "--hop", "512", "--band-edges", "100"], "--band-edges"),
    (["in.wav", "out.pac", "--hop", "512"], "--hop"),
    (["-d", "in.pac", "out.wav", "--band-edges", "0,100"], "--band-edges"),
])
def test_cli_refuses_band_energy_arguments_that_make_no_sense(argv, text, capsys):
    """before a file is read: a.pac does not exist"""
    from mrcaudiocodec_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2 and text in capsys.readouterr().err


def test_check_band_energies_args():
    from mrcaudiocodec_amd import cli
    assert cli.check_band_energies_args(False, None, None, {}) is None
    assert cli.check_band_energies_args(True, 512, None, {}) == (512, None)
    hop, edges = cli.check_band_energies_args(True, 100, "0,50.5,2e3", {})
    assert hop == 100 and edges.tolist() == [0.0, 50.5, 2000.0]
    for flag in cli.BAND_ENERGIES_REFUSES:
        with pytest.raises(ValueError, match="does not go with %s" % flag):
            cli.check_band_energies_args(True, 512, None, {flag: True})
    assert "src" not in cli.BAND_ENERGIES_REFUSES and "-d" in cli.BAND_ENERGIES_REFUSES


# ------------------------------------------------------------------ what the estimate resolves
TONES = ((0.25, 1000.0), (0.075, 5200.0))


def _tone_probe(seed):
    """Oracle transforms only, no quantiser: L = 1024, S = 128, 40 hops of which 20 % are short at random; a 0.25 tone at
    1 kHz and a 0.075 tone at 5.2 kHz over 0.01 white noise; frames of 4096 samples, the 25 critical bands.
    -> (est [25][10], true frame totals [10], the tone bands)"""
    L, S, hops, fs, hop = 1024, 128, 40, 48000, 4096
    rng = np.random.default_rng(seed)
    short = rng.random(hops) < 0.2
    n = hops * L
    t = np.arange(n)
    x = sum(A * np.sin(2 * np.pi * f / fs * t) for A, f in TONES) + 0.01 * rng.standard_normal(n)
    seq = LR.block_sequence(hops + 1, list(short) + [False], L, S)
    lines = LR.analyse(x, seq, L)
    edges = BR.critical_edges(fs)
    B = np.array([BR.band_sums(X, BR.line_ranges(fs, a, b, edges)) for (p, a, b), X in zip(seq, lines)])
    est, _ = BR.frames(seq, B, L, 0, n // hop, hop)
    true = (x * x).reshape(-1, hop).sum(axis=1)
    bands = [int(np.searchsorted(edges, f, side="right")) - 1 for _, f in TONES]
    return est, true, bands, hop


def test_tone_bands_read_the_tones_energy():
    """Held: 2 dB on the two bands that hold the tones, against A^2 / 2 * hop, on every frame of seeds 0-4: the bound the
    feature's probe set (twice its 1.01 dB, the margin for seeds not tried).  This construction measures up to 1.36 dB at
    1 kHz (seed 0) and 0.93 dB at 5.2 kHz, and a frame's total within 7.9 % of the true total ("Band energies",
    has the table).  Nothing is asserted on the other bands: they carry the window's leakage."""
    worst, worst_total = 0.0, 0.0
    for seed in range(5):
        est, true, bands, hop = _tone_probe(seed)
        assert bands == [8, 18]
        for (A, f), q in zip(TONES, bands):
            err = np.abs(10 * np.log10(est[q] / (A * A / 2 * hop)))
            print("seed %d, %g Hz in band %d: largest error %.3f dB over %d frames" % (seed, f, q, err.max(), err.size))
            worst = max(worst, err.max())
        total = np.abs(est.sum(axis=0) / true - 1.0).max()
        print("seed %d: a frame's total is within %.1f %% of the true total" % (seed, 100 * total))
        worst_total = max(worst_total, total)
    print("largest tone-band error %.3f dB; largest error of a frame's total %.1f %%" % (worst, 100 * worst_total))
    assert worst <= 2.0


# ------------------------------------------------------------------ the full-coverage identity
@pytest.mark.parametrize("nch", [2, 1])
def test_full_coverage_adds_up_to_the_block_energies_and_the_decoded_signal(nch):
    """edges [0, fs / 2], frames of L / 2 from -L / 2 to the last tile's end: every tile lies under the frames whole, so the sum
    over bands and frames is the sum of the block energies, which is the decoded signal's sum of squares (Parseval; the
    levels tests' 1e-12 for the same identity)"""
    L, S, fs = 1024, 128, 48000
    buf = LR.silent_ends_file(nch, 31 + nch)
    fb = BR.FileBands(buf, S, (1, 1), L, fs)
    p, a, b = fb.blocks[-1]
    end2 = BR.tile2(p, a, b, L)[1]
    assert BR.tile2(*fb.blocks[0], L)[0] == -L and end2 % L == 0
    n_frames = (end2 + L) // L                                       # (end - (-L / 2)) / (L / 2)
    out, needed = fb.window([0.0, fs / 2.0], -L // 2, n_frames, L // 2)
    assert out.shape == (nch, 1, n_frames) and needed == list(range(len(fb.blocks)))
    _, _, e, _ = LR.block_energies(buf, S, (1, 1), 1)
    x = RR.decode(buf, S, (1, 1), 1)
    for c in range(nch):
        got, blocks, signal = out[c].sum(), e[:, c].sum(), (x[c] ** 2).sum()
        print("%d channel(s), channel %d: against the block energies %.3g, against the signal %.3g"
              % (nch, c, abs(got - blocks) / blocks, abs(got - signal) / signal))
        assert signal > 1.0 and abs(got - blocks) <= 1e-12 * blocks and abs(got - signal) <= 1e-12 * signal
    # one frame fewer at either end loses energy only where a tile is cut: frames outside every tile are +0.0
    far, none = fb.window([0.0, fs / 2.0], end2 // 2 + 1, 3, 700)
    assert none == [] and not far.any() and not np.signbit(far).any()
