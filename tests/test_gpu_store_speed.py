"""
GPU tests of the store's windows with a resample ratio per term (mrc_pac_store_decode_window_speeds, PacStore.decode_window /
decode_window_sum(speed_factors=, speed_index=), cli -d --speed): one-term rows against the existing single-ratio call in all
three formats; rows of mixed ratios, with and without per-term band gains, against the NumPy fold of the store's own EXISTING
float64 windows (tests/speed_restatement.py), bit for bit; a call whose terms all name one ratio against decode_window_sum;
independence of the items' order, of company and of the slab size; that work follows each term's own span; damage inside and
outside a span; the cache of tap tables; the library's refusals; the command line.  Files: those of
tests/test_gpu_store_reduced.py, the smallest that hold every block shape, a non-joint last block and both channel counts.
"""
import re
import struct

import numpy as np
import pytest

import chain_kit as kit  # noqa: F401
from chain_kit import handles_closed_after_module  # noqa: F401
import speed_restatement as SP
import sum_restatement as SR
from oracle import decode as odec

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIDS = ("default", "B")
SLAB_OPTION, SLAB_DEFAULT = 7, 1 << 24
ROLLOFF, ZEROS = 0.9475, 16
TERM_COUNTS = (0, 1, 2, 4, 5, 9)
WINDOWS = (1, 255, 256, 257, 700)                    # the workgroup's tile of 256 outputs: below, at and above its edge
GAINS = (1.0, -1.0, 0.0, 0.3, 1e-3, 3.7)             # (tests/test_gpu_store_sum.py's)
MIXES = (None, "mid", "left")
# rate_divisor -> the list of ratios (up, down): 48 kHz at 16 kHz at speeds 1, 9/10, 11/10; up 1, 2 and general, down > up and
# up > down, and the unit ratio; eight, the most a call takes
LISTS = {2: [(2, 3), (20, 27), (20, 33)],
         1: [(1, 1), (3, 2), (1, 3), (160, 441), (2, 3)],
         4: [(1, 1), (8, 1), (3, 2), (2, 3), (4, 5), (5, 4), (7, 8), (160, 147)]}

_KITCHENS = {}


def _kitchen_of(sid):
    from test_gpu_store_reduced import _Kitchen
    if sid not in _KITCHENS:
        _KITCHENS[sid] = _Kitchen(sid)
    return _KITCHENS[sid]


@pytest.fixture(scope="module", params=SIDS)
def kitchen(request):
    return _kitchen_of(request.param)


@pytest.fixture(scope="module", autouse=True)
def stores_closed_after_module():
    yield
    for k in _KITCHENS.values():
        k.store.close()
    _KITCHENS.clear()


def _speed_kw(D):
    """the Python arguments that give LISTS[D]: at D = 2 the base ratio 2 / 3 at speeds 1, 9/10 and 11/10; else no base ratio and
    the speed down / up for the ratio up / down"""
    from mrcaudiocodec_amd.store import speed_ratios
    if D == 2:
        kw = dict(resample=(2, 3, ZEROS, ROLLOFF), speed_factors=[(1, 1), (9, 10), (11, 10)])
    else:
        kw = dict(resample=(1, 1, ZEROS, ROLLOFF), speed_factors=[(down, up) for (up, down) in LISTS[D]])
    assert speed_ratios(kw["resample"], kw["speed_factors"]) == LISTS[D]
    return kw


def _w(ratio):
    from mrcaudiocodec_amd.store import resample_taps
    return 0 if SP.is_unit(ratio) else resample_taps(ratio[0], ratio[1], ZEROS, ROLLOFF)[0]


def _candidates(k, D, ratio, window):
    """(file, start) at one ratio, and how many of them lie wholly past the end (the last ones): the recipe of
    tests/test_gpu_store_resample.py's _items -- every block boundary of the rate divisor's signal mapped to output samples and
    one either side, -37, a window across the file's end, and one wholly past it"""
    up, down = ratio
    W, out, past = _w(ratio), [], []
    for f in range(len(k.files)):
        n = int(k.index[f]["n_samples"]) // D
        out += [(f, b * up // down + d) for b in k.boundaries(f, D) for d in (-1, 0, 1)]
        out += [(f, -37), (f, -(-n * up // down) - window // 2)]
        past.append((f, -(-(n + W) * up // down) + 1))
    return out + past, len(past)


def _terms(k, D, window):
    """(file, start, ratio index) of single terms, the ratio indices cycling through the list, and the positions of the terms
    that lie wholly past their file's end"""
    per = [_candidates(k, D, r, window) for r in LISTS[D]]
    out, past = [], []
    for j in range(max(len(c) for c, _ in per)):
        for r, (c, n_past) in enumerate(per):
            if j < len(c):
                if j >= len(c) - n_past:
                    past.append(len(out))
                out.append((c[j][0], c[j][1], r))
    return out, past


def _items(k, D, window, seed=0):
    """rows of TERM_COUNTS terms in turn until every term of _terms has been used once, shuffled (a row's terms come from
    different files, places and ratios), the gains GAINS in turn"""
    cand, _ = _terms(k, D, window)
    order = np.random.default_rng(seed).permutation(len(cand))
    items, at, g = [], 0, 0
    while at < len(order):
        n = TERM_COUNTS[len(items) % len(TERM_COUNTS)]
        row = []
        for j in order[at:at + n]:
            row.append((cand[j][0], cand[j][1], GAINS[g % len(GAINS)], cand[j][2]))
            g += 1
        items.append(row)
        at += n
    return items


def _call(k, D, items, window, store=None, **kw):
    files, starts, gains, index, offsets = SP.flatten(items)
    return (store or k.store).decode_window_sum(files, starts, gains, window, item_offsets=offsets, rate_divisor=D, speed_index=index,
                                                **dict(_speed_kw(D), **kw))


def _restate(k, D, items, window, mix=None, store=None, **bands):
    return SP.restate(store or k.store, items, window, 2, LISTS[D], ZEROS, ROLLOFF, D, mix, **bands)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int64), b.view(np.int64))


def _same(a, b):
    return torch.equal(a, b) and torch.equal(torch.signbit(a), torch.signbit(b))


# ------------------------------------------------------------------ 1: a one-term row at gain 1.0 is the existing call
@pytest.mark.parametrize("mix", MIXES)
@pytest.mark.parametrize("D", sorted(LISTS))
def test_one_term_rows_are_the_existing_single_ratio_calls(kitchen, D, mix):
    k = kitchen
    channels = 2 if mix is None else None
    for window in WINDOWS:
        terms, past = _terms(k, D, window)
        files, starts, index = map(np.array, zip(*terms))
        assert set(index[:len(LISTS[D])]) == set(range(len(LISTS[D])))           # the indices cycle inside the one call
        for dtype in (torch.float64, torch.float32, torch.int16):
            got = k.store.decode_window(files, starts, window, channels=channels, dtype=dtype, rate_divisor=D, mix=mix,
                                        speed_index=index, **_speed_kw(D)).cpu().numpy()
            want = SP.term_windows(k.store, files, starts, index, window, 2, LISTS[D], ZEROS, ROLLOFF, D, mix, dtype)
            assert got.dtype == want.dtype and got.shape == (len(terms), 2 if mix is None else 1, window)
            assert np.array_equal(got, want), (k.sid, D, mix, window, dtype)
            if dtype == torch.float64:
                assert _same_bits(got, want)
                live = np.setdiff1d(np.arange(len(terms)), past)
                assert np.abs(got[live]).max() > 1e-3            # (signal, not silence)
                assert not got[past].any() and not np.signbit(got[past]).any()       # wholly past the end: +0.0


# ------------------------------------------------------------------ 2: rows of mixed ratios
@pytest.mark.parametrize("mix", MIXES)
@pytest.mark.parametrize("D", sorted(LISTS))
def test_rows_of_mixed_ratios_equal_the_restatement_bit_for_bit(kitchen, D, mix):
    k = kitchen
    channels = 2 if mix is None else None
    for window in WINDOWS:
        items = _items(k, D, window, seed=window)
        assert {len(it) for it in items[:-1]} == set(TERM_COUNTS)                  # (the last row takes what is left)
        assert any(len({r for (_, _, _, r) in it}) > 1 for it in items)           # several ratios in one row
        got = _call(k, D, items, window, channels=channels, dtype=torch.float64, mix=mix).cpu().numpy()
        want = _restate(k, D, items, window, mix)
        assert got.shape == (len(items), 2 if mix is None else 1, window)
        assert _same_bits(got, want), (k.sid, D, mix, window, np.abs(got - want).max())
        assert np.abs(got).max() > 1e-3
        empty = [i for i, it in enumerate(items) if not it]
        assert empty and not got[empty].any() and not np.signbit(got[empty]).any()   # no terms: +0.0


@pytest.mark.parametrize("D", sorted(LISTS))
def test_formats_are_conversions_of_the_f64_rows(kitchen, D):
    k = kitchen
    window = 257
    items = _items(k, D, window, seed=9)
    items.append([(0, 64, 40.0, 0), (0, 64, 40.0, 1), (0, 65, -3.7, 2)])           # past full scale: the 16-bit code saturates
    f64 = _call(k, D, items, window, channels=2, dtype=torch.float64).cpu().numpy()
    i16 = _call(k, D, items, window, channels=2)
    f32 = _call(k, D, items, window, channels=2, dtype=torch.float32)
    assert i16.dtype == torch.int16 and f32.dtype == torch.float32
    assert np.abs(f64[-1]).max() > 1.0 and 0.0 < np.abs(f64[0:-1]).max()
    assert np.array_equal(i16.cpu().numpy(), odec.pcm16(f64))
    assert int(i16[-1].to(torch.int32).abs().max()) == 32767
    assert np.array_equal(f32.cpu().numpy(), f64.astype(np.float32))


# ------------------------------------------------------------------ 3: per-term band gains
@pytest.mark.parametrize("D,mix", [(2, "mid"), (1, None), (4, "left")])
def test_rows_with_per_term_band_gains_equal_the_restatement(kitchen, D, mix):
    from mrcaudiocodec_amd.store import critical_band_edges
    k = kitchen
    n_bands = critical_band_edges(k.h.cfg.sample_rate).size - 1
    rows = [np.ones(n_bands), np.full(n_bands, 0.25), np.random.default_rng(3).uniform(-1.5, 1.5, n_bands)]
    for window in (257, 700):
        items = _items(k, D, window, seed=window + 1)
        n_terms = sum(len(it) for it in items)
        bg = np.stack([rows[j % 3] for j in range(n_terms)])
        got = _call(k, D, items, window, channels=2 if mix is None else None, dtype=torch.float64, mix=mix, band_gains=bg).cpu().numpy()
        want = _restate(k, D, items, window, mix, band_gains=bg)
        assert _same_bits(got, want), (k.sid, D, mix, window, np.abs(got - want).max())
        plain = _restate(k, D, items, window, mix)
        assert np.abs(got).max() > 1e-3 and not _same_bits(got, plain)              # (the gains did something)


# ------------------------------------------------------------------ 4: all terms at one ratio: decode_window_sum
@pytest.mark.parametrize("D", [1, 2])
def test_terms_that_all_name_one_ratio_are_decode_window_sum(kitchen, D):
    from mrcaudiocodec_amd.store import critical_band_edges
    k = kitchen
    window = 300
    n_bands = critical_band_edges(k.h.cfg.sample_rate).size - 1
    for r, ratio in enumerate(LISTS[D]):
        cand, _ = _candidates(k, D, ratio, window)
        cand = cand[::2]
        items, at = [], 0
        while at < len(cand):
            n = TERM_COUNTS[len(items) % len(TERM_COUNTS)]
            items.append([(f, s, GAINS[(at + j) % len(GAINS)], r) for j, (f, s) in enumerate(cand[at:at + n])])
            at += n
        files, starts, gains, _, offsets = SP.flatten(items)
        rs = None if SP.is_unit(ratio) else (ratio[0], ratio[1], ZEROS, ROLLOFF)
        bg = np.random.default_rng(r).uniform(0.0, 2.0, (files.size, n_bands))
        for bands in ({}, dict(band_gains=bg)):
            for dtype in (torch.float64, torch.int16):
                got = _call(k, D, items, window, channels=2, dtype=dtype, **bands)
                want = k.store.decode_window_sum(files, starts, gains, window, item_offsets=offsets, channels=2, dtype=dtype,
                                                 rate_divisor=D, resample=rs, **bands)
                assert torch.equal(got, want) and bool(want.any()), (k.sid, D, ratio, dtype, bool(bands))


# ------------------------------------------------------------------ 5: independence
@pytest.mark.parametrize("D,mix", [(2, None), (1, "mid"), (4, None)])
def test_result_depends_on_the_terms_order_and_on_nothing_else(kitchen, D, mix):
    k = kitchen
    window = 300
    items = _items(k, D, window, seed=4)
    kw = dict(channels=2 if mix is None else None, dtype=torch.float64, mix=mix)
    base = _call(k, D, items, window, **kw)
    assert k.store.stats()["slabs"] == 1
    perm = np.random.default_rng(8).permutation(len(items))
    assert _same(_call(k, D, [items[i] for i in perm], window, **kw), base[torch.from_numpy(perm).to(base.device)])
    for i in range(0, len(items), 5):                            # alone, and in other company
        assert _same(_call(k, D, items[i:i + 1], window, **kw)[0], base[i])
        assert _same(_call(k, D, items[i:i + 3], window, **kw), base[i:i + 3])
    try:
        k.h.set_option(SLAB_OPTION, 1)                           # no two terms fit: every row is its own slab
        got = _call(k, D, items, window, **kw)
        assert k.store.stats()["slabs"] == len(items) and _same(got, base)
        # the rule counts every term at the largest span among the ratios the call's terms name
        two = [[(0, 5, 1.0, 0), (0, 9, 0.3, 1)], [(0, 7, -1.0, 1), (0, 2, 3.7, 0)]] * 4
        span = max(window if SP.is_unit(r) else ((window - 1) * r[1] + r[0] - 1) // r[0] + 2 * _w(r) for r in LISTS[D][:2])
        want = _call(k, D, two, window, **kw)
        k.h.set_option(SLAB_OPTION, 4 * span)                    # two rows of two terms per slab
        got = _call(k, D, two, window, **kw)
        assert k.store.stats()["slabs"] == 4 and _same(got, want)
        k.h.set_option(SLAB_OPTION, 4 * span - 1)                # one term too many: a row per slab
        got = _call(k, D, two, window, **kw)
        assert k.store.stats()["slabs"] == 8 and _same(got, want)
    finally:
        k.h.set_option(SLAB_OPTION, SLAB_DEFAULT)
    rev = [it[::-1] for it in items]                             # the terms' order is part of the definition
    got = _call(k, D, rev, window, **kw).cpu().numpy()
    assert _same_bits(got, _restate(k, D, rev, window, mix))
    assert not _same_bits(got, base.cpu().numpy())               # ... and rounding makes them differ somewhere


# ------------------------------------------------------------------ 6: work follows the spans; damage
@pytest.mark.parametrize("D,mix", [(2, None), (1, "left"), (4, "mid")])
def test_chunks_parsed_are_the_sum_over_the_ratio_groups(kitchen, D, mix):
    k = kitchen
    window = 300
    terms, _ = _terms(k, D, window)
    terms = terms[::3]
    files, starts, index = map(np.array, zip(*terms))
    total, seen = 0, set()
    for r, ratio in enumerate(LISTS[D]):
        sel = index == r
        rs = {} if SP.is_unit(ratio) else dict(resample=(ratio[0], ratio[1], ZEROS, ROLLOFF))
        k.store.decode_window(files[sel], starts[sel], window, rate_divisor=D, mix=mix, **rs)
        total += k.store.stats()["chunks_parsed"]
        seen.add(k.store.stats()["chunks_parsed"])
    assert total > 0 and len(seen) > 1                           # (the spans differ with the ratio)
    k.store.decode_window(files, starts, window, rate_divisor=D, mix=mix, speed_index=index, **_speed_kw(D))
    st = k.store.stats()
    assert st["chunks_parsed"] == total and st["slabs"] == 1 and st["ms"]["window_out"] > 0.0
    far = -(-(int(k.index[0]["n_samples"]) // D + 3000) * 8) - 1                    # past the end at every ratio of the lists
    k.store.decode_window([0, 0], [far, far], window, rate_divisor=D, mix=mix, speed_index=[0, 1], **_speed_kw(D))
    assert k.store.stats()["chunks_parsed"] == 0 and k.store.stats()["decode_launches"] == 0


def test_damage_counts_only_inside_a_terms_own_span(kitchen):
    from mrcaudiocodec_amd import MrcError
    from mrcaudiocodec_amd.store import PacStore
    k = kitchen
    D, ratios = 2, LISTS[2]
    ix, L = k.index[0], k.L
    j = int(ix["n_blocks"]) - 2                                   # the last joint block
    bad = bytearray(k.files[0])
    at = int(ix["chunk_offset"][j, 0]) + 4
    bad[at] = (bad[at] & 0x0F) | 0x40                             # table id 4
    with PacStore(k.h, [k.files[0], bytes(bad)]) as store:
        # windows over the file's first samples do not need block j at any ratio of the list (the slowest reads furthest)
        w = 8
        last = max((7 + w - 1) * down // up + _w((up, down)) for (up, down) in ratios)
        assert int(ix["block_start"][j]) // D >= last + 1 + L // D
        items = [[(0, 7, 1.0, 0), (1, 0, 0.3, 1)], [(1, 3, -1.0, 2), (0, -5, 3.7, 1)]]
        sound = [[(0, s, g, r) for (_, s, g, r) in it] for it in items]
        got = _call(k, D, items, w, store=store, dtype=torch.float64)
        assert store.stats()["chunks_parsed"] > 0
        assert _same(got, _call(k, D, sound, w, dtype=torch.float64)) and bool(got.any())
        for r, (up, down) in enumerate(ratios):                   # inside the damaged block, in that ratio's output samples
            inside = ((int(ix["block_start"][j]) - L) // D) * up // down
            with pytest.raises(MrcError, match=r"mrc_pac_store_decode_window_speeds: file 1: chunk at byte %d: %s"
                               % (at - 4, re.escape("table id not in {0..3, 15}"))) as e:
                _call(k, D, [[(0, 7, 1.0, 0), (1, inside, 0.0, r)]], 3, store=store, dtype=torch.float64)
            assert e.value.code == -1
            assert bool(_call(k, D, [[(0, 7, 1.0, 0), (0, inside, 0.5, r)]], 3, store=store, dtype=torch.float64).any())


# ------------------------------------------------------------------ 7: the cache of tap tables
def test_a_list_of_eight_after_twelve_other_ratios_on_the_handle():
    """the handle's cache holds 16 tables and is emptied when full: with twelve in it, the seven filters of a list of eight must
    all be resolved before any is used, none evicted while a later one is resolved"""
    from mrcaudiocodec_amd import Handle
    from mrcaudiocodec_amd.store import PacStore
    k = _kitchen_of("default")
    D, window = 4, 300
    h = Handle(sample_rate=48000, device_id=0)                   # a handle of its own: an empty cache
    try:
        with PacStore(h, k.files) as store:
            others = [(p, 17) for p in (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14)]
            assert len(others) == 12 and not set(others) & set(LISTS[D])
            for r in others:
                assert bool(store.decode_window([0], [0], 64, rate_divisor=D, resample=r).any())
            items = _items(k, D, window, seed=5)
            got = _call(k, D, items, window, store=store, channels=2, dtype=torch.float64).cpu().numpy()
            want = _restate(k, D, items, window, store=store)
            assert _same_bits(got, want) and np.abs(got).max() > 1e-3
            again = _call(k, D, items, window, store=store, channels=2, dtype=torch.float64).cpu().numpy()
            assert _same_bits(again, want)
    finally:
        h.close()


# ------------------------------------------------------------------ 8: the library's refusals
def _raw(k, D=1, mix=3, ups=(1, 2), downs=(1, 3), n_ratios=None, zeros=16, rolloff=0.9, n_bands=0, edges=None, band_gain=None,
         offsets=(0, 2), files=(0, 0), starts=(0, 9), gains=(1.0, 0.5), ratio_of=(0, 1), window=16, channels=2, fmt=None, out="tensor",
         n_items=None):
    """the entry point itself -> (status, the pre-filled tensor)"""
    from mrcaudiocodec_amd import _lib
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)
    ups, downs, ratio_of = arr(ups, np.int32), arr(downs, np.int32), arr(ratio_of, np.int32)
    offsets, files, starts = arr(offsets, np.int64), arr(files, np.int64), arr(starts, np.int64)
    gains, edges, band_gain = arr(gains, np.float64), arr(edges, np.float64), arr(band_gain, np.float64)
    ptr = lambda a: None if a is None else a.ctypes.data
    n = (offsets.size - 1 if offsets is not None else 1) if n_items is None else n_items
    t = torch.full((max(n, 1), channels if channels in (1, 2) else 2, window if 0 < window <= 4096 else 16), 77, dtype=torch.float64,
                   device=torch.device("cuda", 0))
    rc = _lib.lib.mrc_pac_store_decode_window_speeds(
        k.store._s, D, mix, (ups.size if ups is not None else 1) if n_ratios is None else n_ratios, ptr(ups), ptr(downs), zeros, rolloff,
        n_bands, ptr(edges), ptr(band_gain), n, ptr(offsets), ptr(files), ptr(starts), ptr(gains), ptr(ratio_of), window, channels,
        _lib.MRC_WINDOW_F64 if fmt is None else fmt, t.data_ptr() if out == "tensor" else None, None)
    return rc, t


def test_library_refusals_come_before_any_device_work(kitchen):
    from mrcaudiocodec_amd import _lib
    k = kitchen
    MID = _lib.MRC_MIX_MID
    fn = "mrc_pac_store_decode_window_speeds: "
    band = dict(n_bands=2, edges=[0.0, 1000.0, 8000.0], band_gain=[[1.0, 0.5], [2.0, 1.0]])
    cases = [
        # the refusals of the existing calls and of _sum
        (dict(D=3), ("rate_divisor 3",)), (dict(D=0), ("rate_divisor 0",)), (dict(mix=7), ("mix 7", "MRC_MIX_EACH (3)")),
        (dict(mix=MID), ("n_channels_out must be 1",)), (dict(channels=3), ("n_channels_out",)),
        (dict(channels=1), ("term 0: file 0 is stereo",)),
        (dict(files=[0, len(k.files)]), ("file[1]", "outside the store")), (dict(files=[-1, 0]), ("file[0]", "outside the store")),
        (dict(window=-1), ("window",)), (dict(window=(1 << 40) + 1), ("window",)), (dict(fmt=9), ("format 9",)),
        (dict(out=None), ("out is NULL",)),
        (dict(offsets=None, n_items=1), ("term_offset is NULL",)), (dict(offsets=[1, 2]), ("term_offset[0] = 1",)),
        (dict(offsets=[0, 2, 1, 2]), ("term_offset decreases at [2]",)), (dict(n_items=-1), ("n_items < 0",)),
        (dict(files=None), ("file, start or gain is NULL",)), (dict(gains=None), ("file, start or gain is NULL",)),
        (dict(gains=[1.0, float("nan")]), ("gain of term 1 is not finite",)),
        # ... of _shaped
        (dict(band, n_bands=257), ("n_bands 257",)), (dict(band, n_bands=-1), ("n_bands -1",)),
        (dict(band, edges=[0.0, 9000.0, 8000.0]), ("edge_hz is not strictly increasing at [2]",)),
        (dict(band, edges=None), ("edge_hz or band_gain is NULL",)), (dict(band, band_gain=None), ("edge_hz or band_gain is NULL",)),
        (dict(band, band_gain=[[1.0, 0.5], [float("inf"), 1.0]]), ("band_gain of term 1, band 0 is not finite",)),
        # ... and this call's own
        (dict(edges=[0.0, 1000.0]), ("n_bands is 0", "edge_hz or band_gain")), (dict(band_gain=[[1.0], [1.0]]), ("n_bands is 0",)),
        (dict(n_ratios=0), ("n_ratios 0", "1..8")), (dict(n_ratios=9), ("n_ratios 9", "1..8")), (dict(n_ratios=-1), ("n_ratios -1",)),
        (dict(ups=None, n_ratios=2), ("ratio_up, ratio_down or ratio_of is NULL",)),
        (dict(downs=None), ("ratio_up, ratio_down or ratio_of is NULL",)),
        (dict(ratio_of=None), ("ratio_up, ratio_down or ratio_of is NULL",)),
        (dict(ups=[1, 0]), ("ratio 1: up 0",)), (dict(downs=[-3, 3]), ("ratio 0: down -3",)),
        (dict(ups=[1, 1], downs=[1, 9]), ("ratio 1: down 9", "8 * up")), (dict(ups=[9, 2], downs=[1, 3]), ("ratio 0: up 9", "8 * down")),
        (dict(ups=[1, 1025], downs=[1, 1024]), ("ratio 1: up 1025",)), (dict(zeros=0), ("ratio 1: zeros 0",)),
        (dict(zeros=65), ("ratio 1: zeros 65",)), (dict(rolloff=0.25), ("ratio 1: rolloff",)),
        (dict(ratio_of=[0, 2]), ("ratio_of of term 1 = 2", "2 ratios")), (dict(ratio_of=[-1, 0]), ("ratio_of of term 0 = -1",)),
    ]
    for change, words in cases:
        rc, out = _raw(k, **change)
        text = _lib.lib.mrc_last_error(k.h._h).decode()
        assert rc == _lib.MRC_ERR_INVALID and bool((out == 77).all()), (change, rc, text)
        assert text.startswith(fn) and all(w in text for w in words), (change, text)
    # nothing to do: MRC_OK, nothing written
    for change in (dict(offsets=[0], files=None, starts=None, gains=None, ratio_of=None), dict(window=0)):
        rc, out = _raw(k, **change)
        assert rc == 0 and bool((out == 77).all()), change
    # ratios that all reduce to 1 do not look at zeros and rolloff; the call as it stands writes every value
    rc, out = _raw(k, ups=[7, 3], downs=[7, 3], zeros=0, rolloff=9.0)
    assert rc == 0 and bool((out != 77).all())
    rc, out = _raw(k, **band)
    assert rc == 0 and bool((out != 77).all())
    rc, out = _raw(k, offsets=[0, 0, 0], files=None, starts=None, gains=None, ratio_of=None)      # rows without terms: +0.0
    assert rc == 0 and not bool(out.any()) and not bool(torch.signbit(out).any())
    # ... but the list is checked wherever it is given: rows without terms do not let an inadmissible ratio through
    rc, out = _raw(k, offsets=[0, 0, 0], files=None, starts=None, gains=None, ratio_of=None, ups=[1, 1], downs=[1, 9])
    text = _lib.lib.mrc_last_error(k.h._h).decode()
    assert rc == _lib.MRC_ERR_INVALID and bool((out == 77).all()) and text.startswith(fn) and "ratio 1: down 9" in text, text


# ------------------------------------------------------------------ 9: the command line
def test_cli_decodes_at_a_speed(tmp_path, capsys):
    from mrcaudiocodec_amd import cli
    from mrcaudiocodec_amd.store import PacStore, speed_ratios
    k = _kitchen_of("default")
    a, b, dst = str(tmp_path / "a.pac"), str(tmp_path / "b.pac"), str(tmp_path / "x.wav")
    for path in (a, b):
        with open(path, "wb") as fp:
            fp.write(k.files[0])
    ratio = speed_ratios((2, 3), [(11, 10)])[0]
    assert ratio == (20, 33)
    n = int(k.store.n_samples_resampled(*ratio, 2)[0])
    assert n == -(-(int(k.index[0]["n_samples"]) // 2) * 20 // 33)
    want = k.store.decode_window([0], [0], n, dtype=torch.int16, rate_divisor=2, mix="mid", resample=ratio)[0].cpu().numpy()
    cli.main(["-d", a, dst, "--speed", "11/10", "--sample-rate", "16000", "--mix", "mid"])
    wav = open(dst, "rb").read()
    assert struct.unpack("<L", wav[24:28])[0] == 16000 and struct.unpack("<H", wav[22:24])[0] == 1
    assert struct.unpack("<L", wav[40:44])[0] == 2 * n
    assert wav == cli.wav_bytes(want, 16000) and want.shape == (1, n) and want.any()
    capsys.readouterr()
    # with an overlay: a two-term call whose second term is at speed 1
    with PacStore(k.h, [k.files[0], k.files[0]]) as store:
        first, length = (int(v[0]) for v in store.source_spans([0], 300, [ratio], [0], 2))
        assert (first, length) == (0, 495)
        g = float(store.levels(2, "mid").gains_for_snr(6.0, [0], [first], [1], [50 * 3 // 2], length)[0])
        want2 = store.decode_window_sum([[0, 1]], [[0, 50]], [[1.0, g]], 300, rate_divisor=2, mix="mid", resample=(2, 3),
                                        speed_factors=[(11, 10), (1, 1)], speed_index=[[0, 1]])[0].cpu().numpy()
        parts = [store.decode_window([f], [s], 300, dtype=torch.float64, rate_divisor=2, mix="mid", resample=r)[0].cpu().numpy()
                 for (f, s, r) in ((0, 0, ratio), (1, 50, (2, 3)))]
        assert np.array_equal(want2, odec.pcm16(SR.fold(parts, [1.0, g])))
    cli.main(["-d", a, dst, "--speed", "11/10", "--sample-rate", "16000", "--mix", "mid", "--samples", "300", "--overlay", b, "--snr-db", "6",
              "--overlay-start", "50"])
    assert open(dst, "rb").read() == cli.wav_bytes(want2, 16000) and want2.shape == (1, 300) and want2.any()
    assert ("%.9g" % g) in capsys.readouterr().out and g != 1.0
