"""
Block energies and level maps (mrc_pac_store_block_energy, PacStore.levels, mrcaudiocodec_amd/levels.py, cli --levels) as far
as a CPU reaches: the identity sum_i e_i == sum_t x[t]^2 on coded files, per channel and for the mid, at every rate divisor
(tests/levels_restatement.py against tests/reduced_restatement.decode and tests/mix_restatement.mid_decode); the kernel's
summation order against a plain sum; LevelMap's tiles, cumulative energy, admissible starts, draws and gains against brute
force; what the estimate resolves, on oracle transforms without a quantiser; the Python-side and command-line refusals,
raised before any library call; the binding.
"""
import numpy as np
import pytest

import chain_kit as kit
import levels_restatement as LR
import mix_restatement as MR
import reduced_restatement as RR
from mrcaudiocodec_amd.levels import LevelMap

SIDS = MR.KIT_SIDS + ("default",)
_E = {}


def _energies(sid, f, D, mid, order="kernel"):
    if (sid, f, D, mid, order) not in _E:
        F = MR.files(sid)
        r = LR.block_energies(F["files"][f], F["S"], F["blksw"], D, mid, order)
        for a in r[1:]:
            a.setflags(write=False)
        _E[(sid, f, D, mid, order)] = r
    return _E[(sid, f, D, mid, order)]


# ------------------------------------------------------------------ the identity on coded files
@pytest.mark.parametrize("D", MR.DIVISORS)
@pytest.mark.parametrize("sid", SIDS)
def test_block_energies_add_up_to_the_decoded_signals_energy(sid, D):
    """Parseval on the orthogonal lapped transform: a rounding bound (1e-12 relative), not a model error.  The decode keeps
    the MDCT's delay, so the identity is whole."""
    F = MR.files(sid)
    worst = 0.0
    for f in range(len(F["files"])):
        nch, blocks, e, _ = _energies(sid, f, D, False)
        x = RR.decode(F["files"][f], F["S"], F["blksw"], D)
        assert e.shape == (len(blocks), nch) and x.shape[0] == nch
        want = (x ** 2).sum(axis=1)
        assert np.all(want > 0)
        rel = np.abs(e.sum(axis=0) - want) / want
        worst = max(worst, rel.max())
        assert rel.max() <= 1e-12, (sid, f, D, rel)
        if nch == 2:
            _, _, em, _ = _energies(sid, f, D, True)
            m = MR.mid_decode(F["files"][f], F["S"], F["blksw"], D)
            want = (m ** 2).sum()
            assert em.shape == (len(blocks), 1)
            rel = abs(em.sum() - want) / want
            worst = max(worst, rel)
            assert rel <= 1e-12, (sid, f, D, rel)
        else:                                                        # a mono file's mid is its channel
            assert np.array_equal(_energies(sid, f, D, True)[2], e)
    print("%s D = %d: largest relative difference %.3g" % (sid, D, worst))


@pytest.mark.parametrize("sid", SIDS)
def test_kernel_order_differs_from_a_plain_sum_by_rounding_alone(sid):
    F = MR.files(sid)
    for f in range(len(F["files"])):
        for D in MR.DIVISORS:
            for mid in (False, True):
                _, _, ek, n = _energies(sid, f, D, mid)
                _, _, ep, _ = _energies(sid, f, D, mid, "plain")
                bound = 2.0 * (n[:, None] + 1) * 2.0 ** -53
                assert np.all(np.abs(ek - ep) <= bound * ep), (sid, f, D, mid)
                assert np.array_equal(ek == 0, ep == 0)


def test_kernel_sum_order():
    """64 lane sums in ascending order, then a balanced tree over the lanes: against an explicit loop"""
    rng = np.random.default_rng(1)
    for n in (1, 31, 64, 65, 200, 1024):
        sq = rng.random(n) * 10.0 ** rng.integers(-12, 3, n)
        lanes = [0.0] * 64
        for k in range(n):
            lanes[k % 64] = lanes[k % 64] + sq[k]
        for width in (1, 2, 4, 8, 16, 32):
            lanes = [lanes[i] + lanes[i + 1] for i in range(0, len(lanes), 2)]
        assert LR.kernel_sum(sq) == lanes[0]
        assert abs(LR.kernel_sum(sq) - np.sum(sq)) <= 2 * (n + 1) * 2.0 ** -53 * np.sum(sq)


# ------------------------------------------------------------------ LevelMap
def _map(sid="default", D=1, mid=False):
    F = MR.files(sid)
    per_file = []
    for f in range(len(F["files"])):
        nch, blocks, e, _ = _energies(sid, f, D, mid)
        total = int(blocks[-1].sum())
        per_file.append(dict(blocks=blocks, energy=e, n_samples=(total - F["L"]) // D))
    return LevelMap(per_file, F["L"], D, F["S"]), per_file


def _brute(per_file, L, D, f, start, window):
    """the overlap of [start, start + window) with every tile, times the tile's energy density"""
    blocks, e = per_file[f]["blocks"], per_file[f]["energy"]
    out = np.zeros(e.shape[1])
    for (p, a, b), row in zip(blocks, e):
        lo, hi = (p + a / 2.0 - L) / D, (p + a + b / 2.0 - L) / D
        overlap = max(0.0, min(hi, start + window) - max(lo, start))
        out += row * (overlap / (hi - lo))
    return out


@pytest.mark.parametrize("D", MR.DIVISORS)
@pytest.mark.parametrize("sid", ["default", "C", "K"])
def test_tiles_and_window_energy(sid, D):
    m, per_file = _map(sid, D)
    L = MR.files(sid)["L"]
    rng = np.random.default_rng(7)
    for f in range(len(m)):
        blocks, e = per_file[f]["blocks"], per_file[f]["energy"]
        edges = m.tiles(f)
        assert edges.dtype == np.float64 and edges.shape == (len(blocks) + 1,)
        assert edges[0] == -L / (2.0 * D) and np.all(np.diff(edges) > 0)      # the first block is (L, .) at 0
        assert edges[-1] == (blocks[-1, 0] + blocks[-1, 1] + blocks[-1, 2] / 2.0 - L) / D
        assert np.array_equal(edges[:-1], (blocks[:, 0] + blocks[:, 1] / 2.0 - L) / D)
        total = e.sum(axis=0)
        assert np.allclose(m.total_energy(f), total, rtol=1e-15, atol=0)
        n = per_file[f]["n_samples"]
        whole = m.window_energy([f], [int(np.floor(edges[0])) - 3], int(edges[-1] - edges[0]) + 8)[0, :e.shape[1]]
        assert np.all(np.abs(whole - total) <= 1e-12 * total)
        for window in (1, 7, MR.files(sid)["S"] // D, n // 3 + 1, n):
            starts = rng.integers(-window - 5, n + 5, 40)
            got = m.window_energy(np.full(40, f), starts, window)
            assert got.shape == (40, m.channels)
            for s, g in zip(starts, got):
                want = _brute(per_file, L, D, f, int(s), window)
                assert np.all(np.abs(g[:len(want)] - want) <= 1e-12 * total), (sid, f, D, s, window)
                if len(want) < m.channels:
                    assert g[1] == g[0]                              # a mono file repeats its channel
        far = m.window_energy([f, f], [int(edges[-1]) + 1, int(edges[0]) - 1 - 50], 50)
        assert not far.any()
        db = m.window_rms_db([f, f], [0, int(edges[-1]) + 1], 64)
        assert np.all(np.isfinite(db[0])) and np.all(np.isneginf(db[1]))
        assert np.array_equal(db[0], 10 * np.log10(m.window_energy([f], [0], 64)[0] / 64))


def test_blocks_that_do_not_follow_one_another_are_refused():
    _, per_file = _map()
    bad = dict(per_file[0], blocks=per_file[0]["blocks"].copy())
    bad["blocks"][2, 0] += 1
    with pytest.raises(ValueError, match="do not follow"):
        LevelMap([bad], 1024, 1, 128)
    with pytest.raises(ValueError, match="must divide"):
        LevelMap(per_file, 1024, 3, 128)


def _silent_hop_map():
    """eight long hops of noise at -20 dB, hop 4 digital silence: oracle analysis, no quantiser"""
    L, S = 1024, 128
    x = 0.1 * np.random.default_rng(11).standard_normal(8 * L)
    x[4 * L:5 * L] = 0.0
    seq = LR.block_sequence(9, [False] * 9, L, S)
    lines = LR.analyse(x, seq, L)
    e = np.array([[(a + b) * float(np.sum(X * X))] for (p, a, b), X in zip(seq, lines)])
    quiet = dict(blocks=np.array(seq), energy=np.zeros_like(e), n_samples=8 * L)
    short = dict(blocks=np.array(seq[:1]), energy=e[:1], n_samples=300)
    return LevelMap([dict(blocks=np.array(seq), energy=e, n_samples=8 * L), quiet, short], L, 1, S), x


def test_admissible_starts_against_a_loop():
    m, x = _silent_hop_map()
    window, floor = 512, -21.5
    want = [s for s in range(0, 8 * 1024 - window + 1, 128) if m.window_rms_db([0], [s], window).max() >= floor]
    got = m.admissible_starts(0, window, floor)
    assert got.dtype == np.int64 and got.tolist() == want
    n_grid = len(range(0, 8 * 1024 - window + 1, 128))
    assert 0 < len(want) < n_grid                                    # both outcomes occur
    # the silent hop [4096, 5120) is shared by the tiles of blocks 4 and 5, [3584, 5632): every window inside them is refused,
    # every window well inside the noise is admitted (the file's two ends are half-empty tiles too)
    assert not any(3584 <= s <= 5120 for s in want)
    assert all(s in want for s in range(1024, 3072 - window + 1, 128)) and all(s in want for s in range(6144, 7168 - window + 1, 128))
    got = m.admissible_starts(0, window, floor, step=100)
    assert got.tolist() == [s for s in range(0, 8 * 1024 - window + 1, 100) if m.window_rms_db([0], [s], window).max() >= floor]
    assert m.admissible_starts(0, 8 * 1024, -60.0).tolist() == [0] and m.admissible_starts(0, 8 * 1024 + 1, -60.0).size == 0
    assert m.admissible_starts(1, window, -200.0).size == 0          # digital silence meets no floor
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="window"):
            m.admissible_starts(0, bad, floor)
        with pytest.raises(ValueError, match="step"):
            m.admissible_starts(0, window, floor, step=bad)
    with pytest.raises(ValueError, match="file"):
        m.admissible_starts(3, window, floor)


def test_sample_starts_and_gains():
    m, x = _silent_hop_map()
    window, floor = 512, -21.5
    files = np.array([0] * 50)
    a = m.sample_starts(files, window, floor, np.random.default_rng(5))
    b = m.sample_starts(files, window, floor, np.random.default_rng(5))
    c = m.sample_starts(files, window, floor, np.random.default_rng(6))
    ok = set(m.admissible_starts(0, window, floor).tolist())
    assert a.dtype == np.int64 and np.array_equal(a, b) and not np.array_equal(a, c)
    assert set(a.tolist()) <= ok and len(set(a.tolist())) > 10
    with pytest.raises(ValueError, match="file 1 "):
        m.sample_starts([0, 1], window, floor, np.random.default_rng(5))
    with pytest.raises(ValueError, match="file 0 "):
        m.sample_starts([0], window, 0.0, np.random.default_rng(5))
    with pytest.raises(ValueError, match="fallback"):
        m.sample_starts([0], window, floor, np.random.default_rng(5), fallback="first")
    with pytest.raises(ValueError, match="Generator"):
        m.sample_starts([0], window, floor, np.random.RandomState(5))
    starts, db = m.grid_levels(0, window)
    got = m.sample_starts([0, 1, 2, 0], window, 0.0, np.random.default_rng(5), fallback="loudest")
    assert got.tolist() == [int(starts[np.argmax(db)]), 0, 0, int(starts[np.argmax(db)])]
    assert db[np.argmax(db)] == m.window_rms_db([0], [got[0]], window).max()
    # gains: the window's level becomes the target; a silent window is left alone
    g = m.gains_to(-26.0, [0, 1, 0], [1024, 0, 9000], window)
    assert g[1] == 1.0 and g[2] == 1.0
    level = m.window_rms_db([0], [1024], window).max()
    assert abs(20 * np.log10(g[0]) + level + 26.0) <= 1e-9
    true_db = 10 * np.log10(np.mean(x[1024:1024 + window] ** 2))
    assert abs(level - true_db) < 1.5                                # stationary noise: the estimate is near the truth


# ------------------------------------------------------------------ what the estimate resolves
def test_resolution_of_the_estimate():
    """Oracle transforms only, no quantiser: L = 1024, S = 128, 60 hops of which 20 % are short at random; Gaussian noise
    whose level changes every 2048 samples, 1e-4 with probability 0.4, else uniform in [0.05, 1] (80 dB steps); 2000 random
    windows per length against the true sum of squares.  Measured on this construction with seed 2: 48 000 samples: largest
    error 0.019 dB; 16 384: largest 0.39 dB; 4 096: 95th percentile 3.4 dB, largest 56 dB (a short window in a quiet stretch
    beside a loud block) -- the figures the bounds were set from (0.01, 0.39; 2.2 and 53).  Held: 0.1 dB and 1 dB; nothing at
    4 096.  The largest error depends on the seed more than those margins suggest: seeds 1, 3 and 2024 gave 0.054, 0.137 and
    0.120 dB at 48 000 and 0.51, 0.62 and 0.88 dB at 16 384 (a window edge inside the tile of a loud block next to a quiet
    one misplaces up to half that block's energy), so 0.1 dB is a bound for this seed, not for the construction."""
    L, S, hops = 1024, 128, 60
    rng = np.random.default_rng(2)
    short = rng.random(hops) < 0.2
    n = hops * L
    level = np.where(rng.random(n // 2048) < 0.4, 1e-4, rng.uniform(0.05, 1.0, n // 2048))
    x = np.repeat(level, 2048) * rng.standard_normal(n)
    seq = LR.block_sequence(hops + 1, list(short) + [False], L, S)
    lines = LR.analyse(x, seq, L)
    e = np.array([[(a + b) * float(np.sum(X * X))] for (p, a, b), X in zip(seq, lines)])
    assert abs(e.sum() - np.sum(x * x)) <= 1e-12 * np.sum(x * x)     # the total is exact
    m = LevelMap([dict(blocks=np.array(seq), energy=e, n_samples=n)], L, 1, S)
    csum = np.concatenate([[0.0], np.cumsum(x * x)])
    worst = {}
    for window in (48000, 16384, 4096):
        starts = rng.integers(0, n - window + 1, 2000)
        est = m.window_energy(np.zeros(2000, np.int64), starts, window)[:, 0]
        true = csum[starts + window] - csum[starts]
        err = np.abs(10 * np.log10(est / true))
        worst[window] = err.max()
        print("window %d: largest error %.4f dB, 95th percentile %.3f dB" % (window, err.max(), np.percentile(err, 95)))
    assert worst[48000] <= 0.1 and worst[16384] <= 1.0


# ------------------------------------------------------------------ Python-side refusals
def _husk(monkeypatch):
    import store_kit
    return store_kit.husk(monkeypatch, handle=False)


def test_levels_refuses_bad_arguments_before_any_library_call(monkeypatch):
    s = _husk(monkeypatch)
    for bad in (0, 3, 8, -2, 2.0, True, "2", None):
        with pytest.raises(ValueError, match="rate_divisor must be an int in"):
            s.levels(rate_divisor=bad)
    for mix in ("left", "right"):
        with pytest.raises(ValueError, match="column of mix=None"):
            s.levels(mix=mix)
    for bad in ("side", "Mid", "", 0, 1, True, b"mid", ("mid",)):
        with pytest.raises(ValueError, match="mix must be None or"):
            s.levels(mix=bad)
    for bad in ([2], [-1], [0, 5]):
        with pytest.raises(ValueError, match="indices into the store"):
            s.levels(files=bad)
    with pytest.raises(ValueError):
        s.levels(files=["a"])


def test_check_levels_mix():
    from mrcaudiocodec_amd import _lib, store
    assert store.check_levels_mix(None) == _lib.MRC_MIX_EACH == 3 and store.check_levels_mix("mid") == _lib.MRC_MIX_MID == 0


@pytest.mark.parametrize("argv,text", [
    (["--levels", "a.pac", "--bits-per-sample", "2.5"], "--levels"),
    (["--levels", "a.pac", "-d"], "--levels"),
    (["--levels", "a.pac", "--mix", "left"], "column"),
    (["--levels", "a.pac", "--mix", "side"], "--mix"),
    (["--levels", "a.pac", "--rate-divisor", "3"], "is not 1, 2 or 4"),
    (["--levels", "a.pac", "--levels-window", "0"], "--levels-window"),
    (["--levels", "a.pac", "--start", "5"], "--levels"),
    (["in.wav", "out.pac", "--levels-window", "100"], "--levels-window"),
    (["--levels"], "--levels"),
])
def test_cli_refuses_levels_arguments_that_make_no_sense(argv, text, capsys):
    """before a file is read: a.pac does not exist"""
    from mrcaudiocodec_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2 and text in capsys.readouterr().err


def test_check_levels_args():
    from mrcaudiocodec_amd import cli
    assert cli.check_levels_args(None, None, {}) is None
    assert cli.check_levels_args(["a.pac", "b.pac"], None, {}) == (["a.pac", "b.pac"], None)
    assert cli.check_levels_args(["a.pac"], 4800, {}) == (["a.pac"], 4800)
    with pytest.raises(ValueError, match="--levels-window.*needs --levels"):
        cli.check_levels_args(None, 4800, {})
    with pytest.raises(ValueError, match="--levels.*-d"):
        cli.check_levels_args(["a.pac"], None, {"-d": True})
    for bad in (0, -5):
        with pytest.raises(ValueError, match="--levels-window"):
            cli.check_levels_args(["a.pac"], bad, {})


# ------------------------------------------------------------------ the binding
def test_binding_of_the_block_energy_call():
    from mrcaudiocodec_amd import _lib
    kit.check_binding(("mrc_pac_store_block_energy",))
    args = kit.header_args("mrc_pac_store_block_energy")
    assert args[:4] == ["mrc_pac_store* s", "int rate_divisor", "int mix", "int64_t n_sel"] and args[-1] == "void* stream"
    text = kit.header_text()
    assert "#define MRC_MIX_EACH" in text and int(text.split("#define MRC_MIX_EACH")[1].split()[0]) == _lib.MRC_MIX_EACH == 3
    assert (_lib.MRC_MIX_MID, _lib.MRC_MIX_LEFT, _lib.MRC_MIX_RIGHT) == (0, 1, 2)
