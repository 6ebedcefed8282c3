"""
The store's weighted sums of windows (mrc_pac_store_decode_window_sum, PacStore.decode_window_sum, LevelMap.gains_for_snr, cli -d
--overlay) as far as a CPU reaches: the restatement's fold (tests/sum_restatement.py) on cases that can be checked by hand;
the Python-side refusals, raised before any library call; the gains for an SNR on a hand-made LevelMap; the command line's
argument checks; the binding.
"""
import numpy as np
import pytest

import chain_kit as kit
import sum_restatement as SR


# ------------------------------------------------------------------ the restatement's fold
def test_fold_of_one_term_at_gain_one_is_the_identity_on_bits():
    rng = np.random.default_rng(3)
    v = rng.standard_normal((2, 300)) * 10.0 ** rng.integers(-300, 300, (2, 300))
    v[0, :4] = [0.0, 5e-324, -5e-324, 1.7976931348623157e308]
    got = SR.fold([v], [1.0])
    assert got.dtype == np.float64 and np.array_equal(got.view(np.int64), v.view(np.int64))


def test_fold_of_no_terms_is_plus_zero():
    got = SR.fold([], [], (2, 7))
    assert got.shape == (2, 7) and got.dtype == np.float64 and not got.any() and not np.signbit(got).any()
    # ... and a fold never ends at -0.0: it starts from +0.0, and x + (-x) is +0.0
    z = SR.fold([np.zeros(3), np.ones(3), np.ones(3)], [-1.0, 2.0, -2.0])
    assert not z.any() and not np.signbit(z).any()


def test_fold_rounds_the_product_then_the_sum_in_term_order():
    from fractions import Fraction
    a, g, c = 1.0 + 2.0 ** -30, 1.0 + 2.0 ** -29, 2.0 ** -53
    # g * a = 1 + 3 * 2^-30 + 2^-59 needs 60 bits: it is rounded before c is added.  The fused form, which rounds once, differs.
    product = float(Fraction(g) * Fraction(a))                   # (Fraction -> float rounds once, to nearest even)
    assert Fraction(product) != Fraction(g) * Fraction(a)
    got = float(SR.fold([np.array([c]), np.array([a])], [1.0, g])[0])
    assert got == float(Fraction(c) + Fraction(product)) and got != float(Fraction(c) + Fraction(g) * Fraction(a))
    # three terms whose sum depends on the order: (big + small) - big loses the small one, (big - big) + small keeps it
    big, small = np.array([1e16]), np.array([1.0])
    assert float(SR.fold([big, small, big], [1.0, 1.0, -1.0])[0]) == 0.0
    assert float(SR.fold([big, big, small], [1.0, -1.0, 1.0])[0]) == 1.0
    with pytest.raises(ValueError, match="fold"):
        SR.fold([big], [1.0, 2.0])


def test_flatten():
    files, starts, gains, offsets = SR.flatten([[(0, 5, 1.0), (2, -3, 0.5)], [], [(1, 7, -1.0)]])
    assert files.tolist() == [0, 2, 1] and starts.tolist() == [5, -3, 7] and gains.tolist() == [1.0, 0.5, -1.0]
    assert offsets.tolist() == [0, 2, 2, 3] and offsets.dtype == files.dtype == np.int64 and gains.dtype == np.float64


# ------------------------------------------------------------------ Python-side checks
def _husk(monkeypatch):
    import store_kit
    return store_kit.husk(monkeypatch, handle=False)


@pytest.mark.parametrize("args,kw,text", [
    (([[0, 1]], [[0]], [[1.0, 1.0]], 16), {}, "must have one shape"),
    (([[0, 1]], [[0, 0]], [[1.0]], 16), {}, "must have one shape"),
    (([0, 1], [0, 0], [1.0, 1.0], 16), {}, r"must be \[n\]\[K\], or 1-D with item_offsets"),
    (([[[0]]], [[[0]]], [[[1.0]]], 16), {}, r"must be \[n\]\[K\]"),
    (([[0, 1]], [[0, 0]], [[1.0, 1.0]], 16), dict(item_offsets=[0, 2]), "must be 1-D"),
    (([0, 1], [0, 0], [1.0, 1.0], 16), dict(item_offsets=[1, 2]), "start at 0"),
    (([0, 1], [0, 0], [1.0, 1.0], 16), dict(item_offsets=[0, 2, 1, 2]), "not decrease"),
    (([0, 1], [0, 0], [1.0, 1.0], 16), dict(item_offsets=[]), "item_offsets must be"),
    (([0, 1], [0, 0], [1.0, 1.0], 16), dict(item_offsets=[[0, 2]]), "item_offsets must be"),
    (([0, 1], [0, 0], [1.0, 1.0], 16), dict(item_offsets=[0, 1]), "end at 1, there are 2 terms"),
    (([0, 1], [0, 0], [1.0, 1.0], 16), dict(item_offsets=[0, 3]), "end at 3, there are 2 terms"),
    (([[0, 1]], [[0, 0]], [[1.0, float("nan")]], 16), {}, "gains must be finite, got nan at term 1"),
    (([[0, 1]], [[0, 0]], [[float("inf"), 1.0]], 16), {}, "gains must be finite, got inf at term 0"),
    (([0], [0], [-float("inf")], 16), dict(item_offsets=[0, 1]), "gains must be finite"),
    (([[0]], [[0]], [[1.0]], 16), dict(rate_divisor=3), "rate_divisor must be an int"),
    (([[0]], [[0]], [[1.0]], 16), dict(rate_divisor=2.0), "rate_divisor must be an int"),
    (([[0]], [[0]], [[1.0]], 16), dict(mix="side"), "mix must be None"),
    (([[0]], [[0]], [[1.0]], 16), dict(mix="mid", channels=2), "channels must be None or 1"),
    (([[0]], [[0]], [[1.0]], 16), dict(resample=(2,)), "resample must be None"),
    (([[0]], [[0]], [[1.0]], 16), dict(resample=(0, 3)), "up must be a positive int"),
    (([[0]], [[0]], [[1.0]], 16), dict(resample=(1, 9)), "is outside"),
    (([[0]], [[0]], [[1.0]], 16), dict(resample=(2, 3, 65, 0.9)), "zeros must be an int"),
    (([[0]], [[0]], [[1.0]], 16), dict(dtype="float32"), "dtype must be torch.int16, torch.float32 or torch.float64"),
])
def test_bad_arguments_are_refused_before_any_library_call(monkeypatch, args, kw, text):
    pytest.importorskip("torch")
    s = _husk(monkeypatch)
    with pytest.raises(ValueError, match="decode_window_sum: .*" + text):
        s.decode_window_sum(*args, **kw)


# ------------------------------------------------------------------ the gains for an SNR
def _hand_made_map():
    from mrcaudiocodec_amd.levels import LevelMap
    blocks = [(8 * i, 8, 8) for i in range(6)]                   # L = 8: tiles [8 i - 4, 8 i + 4)
    rng = np.random.default_rng(5)
    return LevelMap([dict(blocks=blocks, energy=rng.uniform(0.1, 3.0, (6, 2)), n_samples=40),
                     dict(blocks=blocks, energy=rng.uniform(1e-6, 1e-3, (6, 1)), n_samples=40),
                     dict(blocks=blocks, energy=np.zeros((6, 2)), n_samples=40)], 8, 1, 4)


@pytest.mark.parametrize("snr_db", [-12.5, 0.0, 3.0, 20.0, 60.0])
def test_gains_for_snr_realise_the_ratio(snr_db):
    m = _hand_made_map()
    files_a, starts_a = np.array([0, 0, 1, 0, 1]), np.array([0, 7, 3, -2, 11])
    files_b, starts_b = np.array([1, 0, 0, 1, 1]), np.array([5, 20, 9, 30, 2])
    window = 13
    g = m.gains_for_snr(snr_db, files_a, starts_a, files_b, starts_b, window)
    assert g.shape == (5,) and g.dtype == np.float64 and np.all(g > 0) and np.all(np.isfinite(g))
    e_a = m.window_energy(files_a, starts_a, window).sum(axis=1)     # (a mono file counts in both channels, as it sounds)
    e_b = m.window_energy(files_b, starts_b, window).sum(axis=1)
    target = 10.0 ** (snr_db / 10.0)
    realised = e_a / (g * g * e_b)
    print("snr %g dB: max relative error of the realised ratio %.3g" % (snr_db, np.abs(realised / target - 1).max()))
    # sqrt, a division and two products, each within half an ulp (1.1e-16): a few ulps on the squared factor
    assert np.abs(realised / target - 1.0).max() <= 1e-12
    assert np.array_equal(g, np.sqrt(e_a / (e_b * 10.0 ** (snr_db / 10.0))))


def test_gains_for_snr_are_one_where_a_window_is_silent():
    m = _hand_made_map()
    assert m.gains_for_snr(10.0, [2], [0], [0], [0], 13).tolist() == [1.0]         # a silent a
    assert m.gains_for_snr(10.0, [0], [0], [2], [0], 13).tolist() == [1.0]         # a silent b
    assert m.gains_for_snr(10.0, [0, 0], [500, 0], [1, 1], [0, -500], 13).tolist() == [1.0, 1.0]   # outside every tile
    assert m.gains_for_snr(10.0, [], [], [], [], 13).shape == (0,)
    with pytest.raises(ValueError, match="gains_for_snr"):
        m.gains_for_snr(10.0, [0, 0], [0, 0], [1], [0], 13)
    with pytest.raises(ValueError, match="window"):
        m.gains_for_snr(10.0, [0], [0], [1], [0], 0)


# ------------------------------------------------------------------ the command line
def test_check_overlay_args():
    from mrcaudiocodec_amd import cli
    assert cli.check_overlay_args(None, None, None, False) is None and cli.check_overlay_args(None, None, None, True) is None
    assert cli.check_overlay_args("b.pac", "10", None, True) == ("b.pac", 10.0, 0)
    assert cli.check_overlay_args("b.pac", -3.5, -4800, True) == ("b.pac", -3.5, -4800)
    with pytest.raises(ValueError, match="--overlay.*needs -d"):
        cli.check_overlay_args("b.pac", "10", None, False)
    with pytest.raises(ValueError, match="--overlay needs --snr-db"):
        cli.check_overlay_args("b.pac", None, None, True)
    with pytest.raises(ValueError, match="--snr-db belongs to --overlay"):
        cli.check_overlay_args(None, "10", None, True)
    with pytest.raises(ValueError, match="--overlay-start belongs to --overlay"):
        cli.check_overlay_args(None, None, 5, True)
    for bad in ("loud", "nan", "inf", float("-inf")):
        with pytest.raises(ValueError, match="--snr-db"):
            cli.check_overlay_args("b.pac", bad, None, True)
    for bad in (1.5, True, "7"):
        with pytest.raises(ValueError, match="--overlay-start"):
            cli.check_overlay_args("b.pac", "10", bad, True)


@pytest.mark.parametrize("argv,text", [
    (["in.wav", "out.pac", "--overlay", "b.pac", "--snr-db", "10"], "--overlay adds a second .pac file under a decode: it needs -d"),
    (["-d", "in.pac", "out.wav", "--overlay", "b.pac"], "--overlay needs --snr-db"),
    (["-d", "in.pac", "out.wav", "--snr-db", "10"], "--snr-db belongs to --overlay"),
    (["-d", "in.pac", "out.wav", "--overlay-start", "10"], "--overlay-start belongs to --overlay"),
    (["-d", "in.pac", "out.wav", "--overlay", "b.pac", "--snr-db", "loud"], "--snr-db: 'loud' is not a number"),
    (["--levels", "a.pac", "--overlay", "b.pac", "--snr-db", "10"], "--overlay"),
])
def test_cli_refuses_an_overlay_that_makes_no_sense(argv, text, capsys):
    from mrcaudiocodec_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2 and text in capsys.readouterr().err


# ------------------------------------------------------------------ the binding
def test_binding_of_the_sum_call():
    kit.check_binding(("mrc_pac_store_decode_window_sum",))
    args = kit.header_args("mrc_pac_store_decode_window_sum")
    assert args[1:7] == ["int rate_divisor", "int mix", "int up", "int down", "int zeros", "double rolloff"]
    assert [a.split()[-1] for a in args[7:12]] == ["n_items", "term_offset", "file", "start", "gain"]
    assert len(args) == len(kit.header_args("mrc_pac_store_decode_window_resampled")) + 2
