"""
The store's band gains on the MDCT lines (mrc_pac_store_decode_window_shaped, PacStore.decode_window(band_gains=),
store.gains_from_db, store.band_mask_gains, cli -d --band-gains-db) as far as a CPU reaches: the restatement's line-to-band
rule (tests/shape_restatement.py) against the library's mrc_band_line_ranges; the two identities the GPU tests rest on, on the
restatement itself -- gains of 1.0 are reduced_restatement.decode on bits, gains that are all 0.25 or all -2.0 are that factor
times it on bits, at D = 1, 2, 4; the Python-side refusals, raised before any library call; the two helpers on cases that can be
checked by hand; the command line's argument checks; the binding.
"""
import numpy as np
import pytest

import chain_kit as kit
import mix_restatement as MR
import reduced_restatement as RR
import settings_kit as SK
import shape_restatement as SH


def _shapes(L, S):
    return ((L, L), (L, S), (S, S), (S, L))


def _edge_sets(rate, L, S):
    """edge sets in Hz for blocks of L and S lines at `rate`: an edge exactly on a line's frequency (long line 10 and short line
    3), a band narrower than a short block's line spacing, edge[0] > 0, and a last edge below and above Nyquist"""
    f_long = lambda k: (k + 0.5) * ((rate / L) / 2.)
    f_short = lambda k: (k + 0.5) * ((rate / S) / 2.)
    spacing = rate / (2.0 * S)
    return {
        "on_a_line": sorted([0.0, f_long(10), f_short(3), rate / 2.0]),
        "narrow": [f_short(2) + 0.1 * spacing, f_short(2) + 0.4 * spacing, f_short(5), 0.4 * rate],      # band 0: no short line
        "above_zero_below_nyquist": [310.0, 1234.5, 3400.0, 0.31 * rate],
        "above_nyquist": [0.0, 1000.0, 0.75 * rate],
        "one_band": [0.0, rate / 2.0],
    }


# ------------------------------------------------------------------ the line-to-band rule
@pytest.mark.parametrize("sid", ("default",) + MR.KIT_SIDS)
def test_restated_line_ranges_equal_the_librarys(sid):
    from mrcaudiocodec_amd.store import band_line_ranges
    if sid == "default":
        L, S, rate = 1024, 128, 48000
    else:
        (L, S), rate = SK.lengths(sid), int(SK.config(sid).sample_rate)
    sets = _edge_sets(rate, L, S)
    for name, edges in sets.items():
        for a, b in _shapes(L, S):
            want = SH.line_ranges(rate, a, b, edges)
            got = band_line_ranges(rate, a, b, edges)
            assert got.tolist() == want.tolist(), (sid, name, a, b)
            band = SH.line_bands(rate, a, b, edges)                      # ... and the per-line form says the same
            for q in range(len(edges) - 1):
                assert np.flatnonzero(band == q).tolist() == list(range(int(want[q]), int(want[q + 1]))), (sid, name, a, b, q)
            assert np.count_nonzero(band == SH.NO_BAND) == want[0] + (a + b) // 2 - want[-1]
    # the edge on a line's frequency: that line belongs to the band that STARTS there (edge <= f_k)
    long_bands, short_bands = SH.line_bands(rate, L, L, sets["on_a_line"]), SH.line_bands(rate, S, S, sets["on_a_line"])
    assert long_bands[10] == long_bands[9] + 1 == long_bands[11] and short_bands[3] == short_bands[2] + 1 == short_bands[4]
    # the narrow band holds no line of a short block, and lines of a long one
    assert not (SH.line_bands(rate, S, S, sets["narrow"]) == 0).any() and (SH.line_bands(rate, L, L, sets["narrow"]) == 0).any()
    assert SH.line_bands(rate, L, L, sets["above_zero_below_nyquist"])[0] == SH.NO_BAND
    assert SH.line_bands(rate, L, L, sets["above_zero_below_nyquist"])[-1] == SH.NO_BAND
    assert SH.line_bands(rate, L, L, sets["above_nyquist"])[-1] == 1


# ------------------------------------------------------------------ the identities, on the restatement
@pytest.fixture(scope="module")
def default_file():
    F = MR.files("default")
    return F["files"][0], F["S"], F["blksw"]


@pytest.mark.parametrize("D", MR.DIVISORS)
def test_restatement_identities(default_file, D):
    buf, S, blksw = default_file
    edges = _edge_sets(48000, 1024, 128)["on_a_line"]                    # [0, Nyquist]: every line in a band
    plain = RR.decode(buf, S, blksw, D)
    ones = SH.decode(buf, S, blksw, D, 48000, edges, [1.0, 1.0, 1.0])
    assert ones.shape == plain.shape and np.array_equal(ones.view(np.int64), plain.view(np.int64)) and plain.any()
    for g in (0.25, -2.0):
        got = SH.decode(buf, S, blksw, D, 48000, edges, [g, g, g])
        assert np.array_equal(got, g * plain), (D, g, np.abs(got - g * plain).max())
    mid = SH.decode(buf, S, blksw, D, 48000, edges, [1.0, 1.0, 1.0], mid=True)
    want = MR.mid_decode(buf, S, blksw, D)
    assert mid.shape == (1,) + want.shape and np.array_equal(mid[0].view(np.int64), want.view(np.int64))
    assert np.array_equal(SH.decode(buf, S, blksw, D, 48000, edges, [-2.0] * 3, mid=True)[0], -2.0 * want)


def test_restatement_leaves_lines_outside_every_band_alone(default_file):
    buf, S, blksw = default_file
    edges = [310.0, 1234.5, 3400.0, 0.31 * 48000]
    zeros = SH.decode(buf, S, blksw, 1, 48000, edges, [0.0, 0.0, 0.0])
    plain = RR.decode(buf, S, blksw, 1)
    assert zeros.any() and not np.array_equal(zeros, plain)              # what is left: the lines below 310 Hz and above 14880 Hz
    lines = np.arange(1.0, 1025.0)
    got = SH.shape_lines(lines, 48000, 1024, 1024, edges, [0.0, -1.0, 0.5])
    band = SH.line_bands(48000, 1024, 1024, edges)
    assert np.array_equal(got[band == SH.NO_BAND], lines[band == SH.NO_BAND]) and not got[band == 0].any()
    assert np.array_equal(got[band == 1], -lines[band == 1]) and np.array_equal(got[band == 2], 0.5 * lines[band == 2])


# ------------------------------------------------------------------ how exact the restatement itself is
@pytest.mark.parametrize("D", MR.DIVISORS)
def test_the_restatement_against_the_exact_evaluation(default_file, D):
    """oracle.decode.IMDCT rounds a phase of up to 2 pi n0 before it reduces it: about 1e-13 of the amplitude inside the
    transform.  On the default five-hop file that is well inside the 1e-12 of the file's peak the GPU tests hold the device
    to; and the exact evaluation obeys the power-of-two identity as the restatement does."""
    buf, S, blksw = default_file
    planes, blks = SH.blocks(buf, S, blksw)
    one = (48000, [0.0, 24000.0], [1.0])
    ref, exact = SH.synthesise(planes, blks, D, *one), SH.synthesise_exact(planes, blks, D, *one)
    assert exact.dtype == np.longdouble and exact.shape == ref.shape
    own = float(np.abs(ref - exact).max()) / np.abs(ref).max()
    print("D = %d: the NumPy restatement lies %.3g of the file's peak from the exact evaluation" % (D, own))
    assert 0.0 < own <= 2e-13                                            # measured: 1.4e-13, 4.0e-14, 2.4e-14 at D = 1, 2, 4
    quarter = SH.synthesise_exact(planes, blks, D, 48000, [0.0, 24000.0], [0.25])
    assert np.array_equal(quarter, np.longdouble(0.25) * exact)


def test_the_restatement_is_no_reference_for_a_lone_block_whose_aliasing_cancels():
    """setting K's one-block mono file at D = 1: the store keeps the second half of the lone block, whose peak is 14 times
    below the amplitude inside the transform, and the restatement's own error passes 1e-12 of that peak (measured 1.64e-12,
    4.7e-14 absolute) -- which is why tests/test_gpu_store_shape.py holds that one file to the exact evaluation"""
    F = MR.files("K")
    planes, blks = SH.blocks(F["files"][3], F["S"], F["blksw"])
    assert planes == 1 and len(blks) == 1
    one = (48000, [0.0, 24000.0], [1.0])
    ref, exact = SH.synthesise(planes, blks, 1, *one)[:, F["L"]:], SH.synthesise_exact(planes, blks, 1, *one)[:, F["L"]:]
    own, peak = float(np.abs(ref - exact).max()), np.abs(ref).max()
    assert 1e-12 * peak < own < 1e-13 and np.abs(blks[0]["lines"][0]).max() > 2 * peak


# ------------------------------------------------------------------ Python-side checks
from store_kit import husk as _husk


_NAN, _INF = float("nan"), float("inf")


@pytest.mark.parametrize("kw,text", [
    (dict(band_gains=np.ones((2, 24))), r"band_gains must have shape \(2, 25\) or \(25,\)"),
    (dict(band_gains=np.ones((3, 25))), r"band_gains must have shape \(2, 25\)"),
    (dict(band_gains=np.ones((2, 25, 1))), "band_gains must have shape"),
    (dict(band_gains=np.ones(3), band_edges_hz=[0, 100, 200]), r"band_gains must have shape \(2, 2\) or \(2,\)"),
    (dict(band_gains=[["a", "b"], ["c", "d"]], band_edges_hz=[0, 100, 200]), "band_gains must be numbers"),
    (dict(band_gains=[[1.0, None], [1.0, 1.0]], band_edges_hz=[0, 100, 200]), "band_gains must be numbers"),
    (dict(band_gains=[[1.0, 1.0], [1.0, _NAN]], band_edges_hz=[0, 100, 200]), "band_gains must be finite, got nan at unit 1, band 1"),
    (dict(band_gains=[[_INF, 1.0], [1.0, 1.0]], band_edges_hz=[0, 100, 200]), "band_gains must be finite, got inf at unit 0, band 0"),
    (dict(band_gains=[1.0, -_INF], band_edges_hz=[0, 100, 200]), "band_gains must be finite, got -inf at unit 0, band 1"),
    (dict(band_edges_hz=[0, 100, 200]), "band_edges_hz is given without band_gains"),
    (dict(band_gains=[1.0], band_edges_hz=[100]), "band_edges_hz must hold 2 to 257 edges"),
    (dict(band_gains=[1.0, 1.0], band_edges_hz=[0, 200, 100]), "band_edges_hz must start at or above 0 and increase strictly"),
    (dict(band_gains=[1.0], band_edges_hz=[-1, 100]), "band_edges_hz must start at or above 0"),
    (dict(band_gains=[1.0], band_edges_hz=[0, _INF]), "band_edges_hz must be finite"),
    (dict(band_gains=np.ones(257), band_edges_hz=np.arange(258.0)), "band_edges_hz must hold 2 to 257 edges"),
])
def test_bad_band_arguments_are_refused_before_any_library_call(monkeypatch, kw, text):
    pytest.importorskip("torch")
    s = _husk(monkeypatch)
    with pytest.raises(ValueError, match="decode_window: .*" + text):
        s.decode_window([0, 1], [0, 5], 16, **kw)
    sum_kw = dict(kw)
    if "band_gains" in kw and np.ndim(kw["band_gains"]) == 2:            # per term: the shape of files plus the bands
        sum_kw["band_gains"] = [kw["band_gains"]]
    text = text.replace(r"\(2, 25\)", r"\(1, 2, 25\)").replace(r"\(2, 2\)", r"\(1, 2, 2\)")
    with pytest.raises(ValueError, match="decode_window_sum: .*" + text):
        s.decode_window_sum([[0, 1]], [[0, 5]], [[1.0, 0.5]], 16, **sum_kw)


def test_check_band_gains():
    from mrcaudiocodec_amd.store import check_band_gains
    assert check_band_gains(None, (3,), 4, "f") is None
    g = check_band_gains([1, 0, -2.5], (2,), 3, "f")                      # one row for every unit; zero and negative are allowed
    assert g.dtype == np.float64 and g.flags.c_contiguous and g.tolist() == [[1.0, 0.0, -2.5]] * 2
    g = check_band_gains(np.arange(12.0).reshape(2, 2, 3), (2, 2), 3, "f")
    assert g.shape == (4, 3) and g[3].tolist() == [9.0, 10.0, 11.0]
    assert check_band_gains(np.ones((0, 3)), (0,), 3, "f").shape == (0, 3)
    with pytest.raises(ValueError, match="f: band_gains must have shape"):
        check_band_gains(np.ones((2, 3)), (3,), 3, "f")
    with pytest.raises(ValueError, match="f: band_edges_hz is given without band_gains"):
        check_band_gains(None, (3,), 4, "f", [0, 1])


# ------------------------------------------------------------------ the helpers
def test_gains_from_db():
    from mrcaudiocodec_amd.store import gains_from_db
    g = gains_from_db([0.0, 20.0, -20.0, -40.0, -_INF, 6.0])
    assert g.dtype == np.float64 and g[:5].tolist() == [1.0, 10.0, 0.1, 0.01, 0.0] and g[5] == 10.0 ** 0.3
    assert not np.signbit(g[4])
    assert gains_from_db(-_INF) == 0.0 and gains_from_db([[0.0], [-_INF]]).shape == (2, 1)
    for bad in (_INF, _NAN, [0.0, _NAN], "loud", [0.0, 1e9]):
        with pytest.raises(ValueError, match="gains_from_db"):
            gains_from_db(bad)


def test_band_mask_gains():
    from mrcaudiocodec_amd.store import band_mask_gains
    g = band_mask_gains(50, 25, np.random.default_rng(4), n_masks=2, max_width=5)
    assert g.shape == (50, 25) and g.dtype == np.float64 and set(np.unique(g)) <= {0.0, 1.0}
    assert np.array_equal(g, band_mask_gains(50, 25, np.random.default_rng(4), n_masks=2, max_width=5))       # from rng alone
    assert not np.array_equal(g, band_mask_gains(50, 25, np.random.default_rng(5), n_masks=2, max_width=5))
    runs = [np.count_nonzero(np.diff(np.concatenate([[1.0], row, [1.0]])) == -1.0) for row in g]
    assert max(runs) <= 2 and (g == 0).sum(axis=1).max() <= 10 and (g == 0).any() and len({tuple(r) for r in g}) > 10
    one = band_mask_gains(200, 10, np.random.default_rng(1), n_masks=1, max_width=3, floor=0.1)
    assert set(np.unique(one)) == {0.1, 1.0} and (one == 0.1).sum(axis=1).max() == 3
    widths = {int(v) for v in (one == 0.1).sum(axis=1)}
    assert widths == {0, 1, 2, 3}                                         # every width up to max_width is drawn
    # the draws as the docstring has them: per item and mask, the width from [0, max_width], then the first band
    rng = np.random.default_rng(9)
    want = np.ones((3, 8))
    for i in range(3):
        width = int(rng.integers(0, 5))
        first = int(rng.integers(0, 8 - width + 1))
        want[i, first:first + width] = -1.0
    assert np.array_equal(band_mask_gains(3, 8, np.random.default_rng(9), max_width=4, floor=-1.0), want)
    assert np.array_equal(band_mask_gains(4, 6, np.random.default_rng(0), n_masks=0), np.ones((4, 6)))
    assert band_mask_gains(0, 6, np.random.default_rng(0)).shape == (0, 6)
    assert (band_mask_gains(5, 3, np.random.default_rng(0), max_width=99) == 0).sum(axis=1).max() <= 3       # no wider than the row
    for kw in (dict(n_items=-1), dict(n_bands=0), dict(n_bands=257), dict(n_masks=-1), dict(max_width=-1), dict(floor=_NAN),
               dict(rng=7), dict(n_items=2.5)):
        a = dict(n_items=2, n_bands=4, rng=np.random.default_rng(0))
        a.update(kw)
        with pytest.raises(ValueError, match="band_mask_gains"):
            band_mask_gains(**a)


# ------------------------------------------------------------------ the command line
def test_check_band_gains_db_args():
    from mrcaudiocodec_amd import cli
    assert cli.check_band_gains_db_args(None, True) is None and cli.check_band_gains_db_args(None, False) is None
    edges, gains = cli.check_band_gains_db_args("0-300:-inf,3400-24000:-inf", True)
    assert edges.tolist() == [0.0, 300.0, 3400.0, 24000.0] and gains.tolist() == [0.0, 1.0, 0.0]       # the gap: a band at 0 dB
    edges, gains = cli.check_band_gains_db_args("100-200:20,200-400.5:-20", True)
    assert edges.tolist() == [100.0, 200.0, 400.5] and gains.tolist() == [10.0, 0.1]
    edges, gains = cli.check_band_gains_db_args("1000-2000:0", True)
    assert edges.tolist() == [1000.0, 2000.0] and gains.tolist() == [1.0]
    with pytest.raises(ValueError, match="--band-gains-db.*needs -d"):
        cli.check_band_gains_db_args("0-300:-6", False)
    for bad in ("0-300", "300:-6", "0-300:loud", "a-b:0", "0-300:-6,", "300-0:-6", "0-0:1", "0-300:inf", "0-300:nan", "0-inf:0",
                "0-300:-6,200-400:0", "500-600:0,100-200:0", "-5-300:0"):
        with pytest.raises(ValueError, match="--band-gains-db"):
            cli.check_band_gains_db_args(bad, True)
    assert "--band-gains-db" in cli.BAND_ENERGIES_REFUSES


@pytest.mark.parametrize("argv,text", [
    (["in.wav", "out.pac", "--band-gains-db", "0-300:-inf"], "--band-gains-db changes the spectrum of a decode: it needs -d"),
    (["-d", "in.pac", "out.wav", "--band-gains-db", "0-300"], "--band-gains-db: '0-300' is not LO-HI:DB"),
    (["-d", "in.pac", "out.wav", "--band-gains-db", "0-300:0,200-400:0"], "bands ascend and do not overlap"),
    (["--band-energies", "in.pac", "out.npy", "--hop", "512", "--band-gains-db", "0-300:0"], "does not go with --band-gains-db"),
    (["--levels", "a.pac", "--band-gains-db", "0-300:0"], "--band-gains-db"),
    (["-d", "in.pac", "out.wav", "--band-edges", "0,100"], "--band-edges belongs to --band-energies"),
])
def test_cli_refuses_band_gains_that_make_no_sense(argv, text, capsys):
    from mrcaudiocodec_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2 and text in capsys.readouterr().err


# ------------------------------------------------------------------ the binding
def test_binding_of_the_shaped_call():
    kit.check_binding(("mrc_pac_store_decode_window_shaped",))
    args = kit.header_args("mrc_pac_store_decode_window_shaped")
    base = kit.header_args("mrc_pac_store_decode_window_sum")
    assert [a.split()[-1] for a in args[7:10]] == ["n_bands", "edge_hz", "band_gain"] and args[7] == "int n_bands"
    assert args[:7] == base[:7] and args[10:] == base[7:] and len(args) == len(base) + 3
