"""
The store's windows with a resample ratio per term (mrc_pac_store_decode_window_speeds, PacStore.decode_window /
decode_window_sum(speed_factors=, speed_index=), store.speed_ratios, PacStore.source_spans, cli -d --speed) as far as a CPU
reaches: the binding; the arithmetic of the ratios; the source spans against a direct count; the Python-side refusals, raised
before any library call; the command line's argument checks.
"""
from fractions import Fraction

import numpy as np
import pytest

import chain_kit as kit


# ------------------------------------------------------------------ the binding
def test_binding_of_the_speeds_call():
    from mrcaudiocodec_amd import _lib
    kit.check_binding(("mrc_pac_store_decode_window_speeds",))
    assert hasattr(_lib.lib, "mrc_pac_store_decode_window_speeds")
    args = kit.header_args("mrc_pac_store_decode_window_speeds")
    names = [a.split()[-1].lstrip("*") for a in args]
    assert names == ["s", "rate_divisor", "mix", "n_ratios", "ratio_up", "ratio_down", "zeros", "rolloff", "n_bands", "edge_hz",
                     "band_gain", "n_items", "term_offset", "file", "start", "gain", "ratio_of", "window", "n_channels_out", "format",
                     "out", "stream"]
    shaped = [a.split()[-1].lstrip("*") for a in kit.header_args("mrc_pac_store_decode_window_shaped")]
    assert [n for n in names if n not in ("n_ratios", "ratio_up", "ratio_down", "ratio_of")] == \
        [n for n in shaped if n not in ("up", "down")]                   # _shaped's arguments, the one ratio replaced by the list
    assert "#define MRC_MAX_STORE_RATIOS 8" in kit.header_text()


# ------------------------------------------------------------------ the ratios
def test_speed_ratios():
    from mrcaudiocodec_amd.store import MAX_RATIOS, resample_plan, speed_ratios
    d, up, down = resample_plan(48000, 16000)
    assert (d, up, down) == (2, 2, 3)
    assert speed_ratios((up, down), [(9, 10), (1, 1), (11, 10)]) == [(20, 27), (2, 3), (20, 33)]
    assert speed_ratios(None, [(9, 10), (1, 1), (11, 10)]) == [(10, 9), (1, 1), (10, 11)]       # no base ratio: 1 / 1
    assert speed_ratios((4, 6), [(22, 20), (3, 3)]) == [(20, 33), (2, 3)]                       # reduced by the gcd
    assert speed_ratios((2, 3), [(2, 3)]) == [(1, 1)]                                           # ... down to the unit ratio
    assert speed_ratios((2, 3, 8, 0.9), [(1, 2)]) == [(4, 3)]
    for base in (None, (2, 3), (3, 2), (12, 8)):
        for f in ((9, 10), (11, 10), (3, 2), (7, 7)):
            b = Fraction(1) if base is None else Fraction(base[0], base[1])
            want = b / Fraction(f[0], f[1])
            assert speed_ratios(base, [f]) == [(want.numerator, want.denominator)]
    assert MAX_RATIOS == 8 and len(speed_ratios(None, [(1, 1)] * 8)) == 8
    # 44.1 kHz at 16 kHz: 320 / 441; slowed to 10 / 11 it is 352 / 441 and fits, sped up to 11 / 10 it is 3200 / 4851
    assert speed_ratios((320, 441), [(10, 11)]) == [(352, 441)]
    with pytest.raises(ValueError, match=r"speed_ratios: speed_factors\[1\] = 11 / 10 on 320 / 441.*up = 3200 \(of 3200 / 4851, reduced\) is above 1024"):
        speed_ratios((320, 441), [(1, 1), (11, 10)])
    with pytest.raises(ValueError, match=r"speed_factors\[0\] = 9 / 1 on 1 / 1.*up / down = 1 / 9 is outside"):
        speed_ratios(None, [(9, 1)])
    for bad in ([], [(1, 1)] * 9, (1, 1), None, "fast", [(1, 0)], [(0, 1)], [(1.5, 1)], [(True, 1)], [(1, 1, 1)], [7], [(-11, 10)]):
        with pytest.raises(ValueError, match="speed_ratios: speed_factors"):
            speed_ratios((2, 3), bad)
    with pytest.raises(ValueError, match="speed_ratios: resample"):
        speed_ratios((0, 3), [(1, 1)])
    with pytest.raises(ValueError, match="speed_ratios: resample: zeros"):
        speed_ratios((2, 3, 0, 0.9), [(1, 1)])


# ------------------------------------------------------------------ Python-side checks
from store_kit import husk as _husk


def test_source_spans_against_a_direct_count(monkeypatch):
    s = _husk(monkeypatch)
    ratios = [(20, 27), (2, 3), (20, 33), (1, 1), (3, 2)]
    rng = np.random.default_rng(0)
    starts = np.concatenate([rng.integers(-5000, 50000, 200), [0, -1, 1, -37]])
    index = rng.integers(0, len(ratios), starts.size)
    for window in (0, 1, 255, 16000):
        first, length = s.source_spans(starts, window, ratios, index, rate_divisor=2)
        assert first.dtype == np.int64 and length.dtype == np.int64 and first.shape == length.shape == starts.shape
        for k in range(starts.size):
            up, down = ratios[index[k]]
            # output n sits at intermediate time n down / up: the first output's sample, and the samples the window's
            # outputs [start, start + window) lie over, counted one by one
            at = Fraction(int(starts[k]) * down, up)
            assert first[k] == at.numerator // at.denominator
            count = 0
            while Fraction(count * up, down) < window:           # intermediate sample `count` after the start is still under an output
                count += 1
            assert length[k] == count, (window, ratios[index[k]])
    first, length = s.source_spans([[0, 10], [20, 30]], 300, [(20, 33), (2, 3)], [[0, 1], [0, 1]])
    assert first.tolist() == [[0, 15], [33, 45]] and length.tolist() == [[495, 450], [495, 450]]
    for kw, text in ((dict(ratios=[]), "ratios must be a list"), (dict(ratios=[(2, 0)]), "ratios must be a list"),
                     (dict(ratios=[(2, 3, 4)]), "ratios must be a list"), (dict(index=[0, 1, 0]), "speed_index must have shape"),
                     (dict(index=[0, 2]), r"speed_index must lie in 0..1 .* got 2 at unit 1"), (dict(index=[0.0, 1.0]), "speed_index must be ints"),
                     (dict(window=-1), "window must be an int >= 0"), (dict(rate_divisor=3), "rate_divisor")):
        a = dict(starts=[0, 5], window=16, ratios=[(2, 3), (1, 1)], index=[0, 1])
        a.update(kw)
        with pytest.raises(ValueError, match="source_spans: .*" + text):
            s.source_spans(**a)


@pytest.mark.parametrize("kw,text", [
    (dict(speed_factors=[(1, 1)]), "speed_factors and speed_index go together, got only speed_factors"),
    (dict(speed_index=[0, 0]), "speed_factors and speed_index go together, got only speed_index"),
    (dict(speed_factors=[(1, 1)], speed_index=[0]), r"speed_index must have shape \(2,\), got \(1,\)"),
    (dict(speed_factors=[(1, 1)], speed_index=[[0, 0]]), r"speed_index must have shape \(2,\)"),
    (dict(speed_factors=[(1, 1), (9, 10)], speed_index=[0, 2]), r"speed_index must lie in 0..1 .* got 2 at unit 1"),
    (dict(speed_factors=[(1, 1)], speed_index=[-1, 0]), r"speed_index must lie in 0..0 .* got -1 at unit 0"),
    (dict(speed_factors=[(1, 1)], speed_index=[0.0, 0.0]), "speed_index must be ints"),
    (dict(speed_factors=[(1, 1)], speed_index=["a", "b"]), "speed_index must be ints"),
    (dict(speed_factors=[], speed_index=[0, 0]), "speed_factors must be a list of 1 to 8"),
    (dict(speed_factors=[(1, 1)] * 9, speed_index=[0, 0]), "speed_factors must be a list of 1 to 8"),
    (dict(speed_factors=(11, 10), speed_index=[0, 0]), r"speed_factors\[0\] must be a pair of positive ints"),
    (dict(speed_factors=[(1, 1), (11, 0)], speed_index=[0, 0]), r"speed_factors\[1\] must be a pair of positive ints"),
    (dict(speed_factors=[(1.1, 1)], speed_index=[0, 0]), r"speed_factors\[0\] must be a pair of positive ints"),
    (dict(speed_factors=[(11, 10, 1)], speed_index=[0, 0]), r"speed_factors\[0\] must be a pair of positive ints"),
    (dict(speed_factors=[(1, 1), (11, 10)], speed_index=[0, 0], resample=(320, 441)),
     r"speed_factors\[1\] = 11 / 10 on 320 / 441.*up = 3200 \(of 3200 / 4851, reduced\) is above 1024"),
    (dict(speed_factors=[(9, 1)], speed_index=[0, 0]), r"speed_factors\[0\] = 9 / 1 on 1 / 1.*1 / 9 is outside"),
    (dict(speed_factors=[(1, 1)], speed_index=[0, 0], resample=(2, 3, 99, 0.9)), "resample: zeros"),
])
def test_bad_speed_arguments_are_refused_before_any_library_call(monkeypatch, kw, text):
    pytest.importorskip("torch")
    s = _husk(monkeypatch)
    with pytest.raises(ValueError, match="decode_window: .*" + text):
        s.decode_window([0, 1], [0, 5], 16, **kw)
    sum_kw = dict(kw)
    if "speed_index" in kw:                                      # per term: the shape of files
        sum_kw["speed_index"] = [kw["speed_index"]]
    text = text.replace(r"\(2,\)", r"\(1, 2\)").replace(r"got \(1,\)", r"got \(1, 1\)")
    with pytest.raises(ValueError, match="decode_window_sum: .*" + text):
        s.decode_window_sum([[0, 1]], [[0, 5]], [[1.0, 0.5]], 16, **sum_kw)


def test_check_speed_index():
    from mrcaudiocodec_amd.store import check_speed_index
    i = check_speed_index([[0, 2], [1, 1]], (2, 2), 3, "f")
    assert i.dtype == np.int32 and i.flags.c_contiguous and i.tolist() == [0, 2, 1, 1]
    assert check_speed_index(np.zeros(0, np.int64), (0,), 1, "f").shape == (0,)
    assert check_speed_index(np.array([1, 0], np.uint8), (2,), 2, "f").tolist() == [1, 0]
    with pytest.raises(ValueError, match="f: speed_index must have shape"):
        check_speed_index([0, 1], (3,), 2, "f")


# ------------------------------------------------------------------ the command line
def test_check_speed_args():
    from mrcaudiocodec_amd import cli
    assert cli.check_speed_args(None, True) is None and cli.check_speed_args(None, False) is None
    assert cli.check_speed_args("11/10", True) == (11, 10) and cli.check_speed_args("9/10", True) == (9, 10)
    assert cli.check_speed_args("2", True) == (2, 1)
    with pytest.raises(ValueError, match="--speed plays a decode faster or slower: it needs -d"):
        cli.check_speed_args("11/10", False)
    for bad in ("1.1", "11/", "/10", "0/10", "11/0", "-11/10", "11/10/2", "fast", ""):
        with pytest.raises(ValueError, match="--speed: .* is not NUM/DEN"):
            cli.check_speed_args(bad, True)
    assert "--speed" in cli.BAND_ENERGIES_REFUSES


@pytest.mark.parametrize("argv,text", [
    (["in.wav", "out.pac", "--speed", "11/10"], "--speed plays a decode faster or slower: it needs -d"),
    (["-d", "in.pac", "out.wav", "--speed", "1.1"], "--speed: '1.1' is not NUM/DEN"),
    (["-d", "in.pac", "out.wav", "--speed", "0/10"], "--speed: '0/10' is not NUM/DEN"),
    (["--band-energies", "in.pac", "out.npy", "--hop", "512", "--speed", "11/10"], "does not go with --speed"),
    (["--levels", "a.pac", "--speed", "11/10"], "--speed plays a decode faster or slower: it needs -d"),
])
def test_cli_refuses_speeds_that_make_no_sense(argv, text, capsys):
    """before a file is read: in.pac does not exist"""
    from mrcaudiocodec_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2 and text in capsys.readouterr().err
