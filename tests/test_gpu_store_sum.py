"""
GPU tests of the store's weighted sums of windows (mrc_pac_store_decode_window_sum, PacStore.decode_window_sum, cli -d --overlay):
the float64 rows equal, bit for bit, the NumPy fold of the store's own EXISTING float64 windows (tests/sum_restatement.py) --
for every rate divisor, mix, resample ratio, tile edge of the workgroup, term count around the kernel's read-ahead group of
four and start around every block boundary, before the file, across its end and past it; a one-term item at gain 1.0 against
the existing call in all three formats; the other formats as conversions of the call's own float64 rows, saturation included;
the channel map; independence of the items' order, of company and of the slab size, and dependence on the TERMS' order as the
restatement has it; that work follows the terms' windows; damage inside and outside a term's span; the library's refusals;
the command line; linearity.  Files: those of tests/test_gpu_store_reduced.py, the smallest that hold every block shape, a
non-joint last block and both channel counts.
"""
import re

import numpy as np
import pytest

import chain_kit as kit  # noqa: F401
from chain_kit import handles_closed_after_module  # noqa: F401
import resample_restatement as RS
import sum_restatement as SR
from oracle import decode as odec

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIDS = ("default", "B")
SLAB_OPTION, SLAB_DEFAULT = 7, 1 << 24
ROLLOFF, ZEROS = 0.9475, 16
TERM_COUNTS = (0, 1, 2, 4, 5, 9)                     # the read-ahead group of four terms: none, below, at, one past, two groups + 1
WINDOWS = (1, 255, 256, 257, 700)                    # the workgroup's tile of 256 outputs: below, at and above its edge
GAINS = (1.0, -1.0, 0.0, 0.3, 1e-3, 3.7)
MIXES = (None, "mid", "left")
# (rate_divisor, resample)
PLAIN = ((1, None), (2, None), (4, None))
RESAMPLED = ((2, (2, 3)), (1, (1, 3)), (1, (160, 441)), (1, (3, 2)))

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


def _rs(resample):
    return None if resample is None else (resample[0], resample[1], ZEROS, ROLLOFF)


def _candidates(k, D, resample, window):
    """(file, start) of single terms: a start at every block boundary and one either side, -37, a start whose window
    straddles the file's end, and one wholly past it -- in output samples of the call (the boundaries of the rate divisor's
    signal mapped through up / down when resampling)"""
    from mrcaudiocodec_amd.store import resample_taps
    up, down = resample or (1, 1)
    W = resample_taps(up, down, ZEROS, ROLLOFF)[0] if resample else 0
    out = []
    for f in range(len(k.files)):
        n = int(k.index[f]["n_samples"]) // D
        out += [(f, b * up // down + d) for b in k.boundaries(f, D) for d in (-1, 0, 1)]
        out += [(f, -37), (f, -(-n * up // down) - window // 2), (f, -(-(n + W) * up // down) + 1)]
    return out


def _items(k, D, resample, window, seed=0):
    """items of TERM_COUNTS terms in turn until every candidate has been a term once, the candidates shuffled (an item's terms
    come from different files and places), the gains GAINS in turn"""
    cand = _candidates(k, D, resample, window)
    order = np.random.default_rng(seed).permutation(len(cand))
    items, at, g = [], 0, 0
    while at < len(order):
        n = TERM_COUNTS[len(items) % len(TERM_COUNTS)]
        terms = []
        for j in order[at:at + n]:
            terms.append((cand[j][0], cand[j][1], GAINS[g % len(GAINS)]))
            g += 1
        items.append(terms)
        at += n
    return items


def _sum(k, items, window, **kw):
    files, starts, gains, offsets = SR.flatten(items)
    return k.store.decode_window_sum(files, starts, gains, window, item_offsets=offsets, **kw)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int64), b.view(np.int64))


def _same(a, b):
    return torch.equal(a, b) and torch.equal(torch.signbit(a), torch.signbit(b))


# ------------------------------------------------------------------ 1: float64 equals the restatement, bit for bit
@pytest.mark.parametrize("mix", MIXES)
@pytest.mark.parametrize("D,resample", PLAIN + RESAMPLED)
def test_f64_equals_the_restatement_bit_for_bit(kitchen, D, resample, mix):
    k = kitchen
    channels = 2 if mix is None else None
    for window in WINDOWS:
        items = _items(k, D, resample, window, seed=window)
        assert {len(it) for it in items} == set(TERM_COUNTS)
        if len(k.files) > 1:
            assert any(len({f for (f, _, _) in it}) > 1 for it in items)      # terms of different files in one item
        got = _sum(k, items, window, channels=channels, dtype=torch.float64, rate_divisor=D, mix=mix, resample=_rs(resample))
        want = SR.restate(k.store, items, window, 2, D, mix, _rs(resample))
        got = got.cpu().numpy()
        assert got.shape == (len(items), 2 if mix is None else 1, window)
        assert _same_bits(got, want), (k.sid, D, resample, mix, window, np.abs(got - want).max())
        assert np.abs(got).max() > 1e-3                          # (signal, not silence)
        empty = [i for i, it in enumerate(items) if not it]
        assert empty and not got[empty].any() and not np.signbit(got[empty]).any()       # no terms: +0.0


# ------------------------------------------------------------------ 2: a single term at gain 1.0 is the existing call
@pytest.mark.parametrize("D,mix,resample", [(1, None, None), (2, "mid", None), (4, "left", None), (2, None, (2, 3)), (1, "mid", (160, 441))])
def test_one_term_at_gain_one_is_the_existing_call(kitchen, D, mix, resample):
    k = kitchen
    window = 300
    files, starts = map(np.array, zip(*_candidates(k, D, resample, window)))
    kw = dict(channels=2 if mix is None else None, rate_divisor=D, mix=mix, resample=_rs(resample))
    for dtype in (torch.int16, torch.float32, torch.float64):
        want = k.store.decode_window(files, starts, window, dtype=dtype, **kw)
        got = k.store.decode_window_sum(files[:, None], starts[:, None], np.ones((files.size, 1)), window, dtype=dtype, **kw)
        assert got.dtype == dtype and torch.equal(got, want) and bool(want.any())
        if dtype != torch.int16:
            assert not bool(torch.signbit(got)[got == 0].any())


# ------------------------------------------------------------------ 3: the other formats
@pytest.mark.parametrize("D,resample", [(1, None), (2, (2, 3))])
def test_formats_are_conversions_of_the_f64_rows(kitchen, D, resample):
    k = kitchen
    window = 257
    items = _items(k, D, resample, window, seed=9)
    items.append([(0, 64, 40.0), (0, 64, 40.0), (0, 65, -3.7)])                    # past full scale: the 16-bit code saturates
    kw = dict(channels=2, rate_divisor=D, resample=_rs(resample))
    f64 = _sum(k, items, window, dtype=torch.float64, **kw).cpu().numpy()
    i16 = _sum(k, items, window, **kw)
    f32 = _sum(k, items, window, dtype=torch.float32, **kw)
    assert i16.dtype == torch.int16 and f32.dtype == torch.float32
    assert np.abs(f64[-1]).max() > 1.0 and 0.0 < np.abs(f64[0:-1]).max()
    assert np.array_equal(i16.cpu().numpy(), odec.pcm16(f64))
    assert int(i16[-1].to(torch.int32).abs().max()) == 32767
    assert np.array_equal(f32.cpu().numpy(), f64.astype(np.float32))


# ------------------------------------------------------------------ 4: the channel map under MRC_MIX_EACH
def test_a_mono_term_adds_to_both_channels_and_a_stereo_term_needs_two():
    from mrcaudiocodec_amd import MrcError
    k = _kitchen_of("B")
    mono = [f for f in range(len(k.files)) if k.index[f]["n_channels"] == 1][0]
    stereo = [f for f in range(len(k.files)) if k.index[f]["n_channels"] == 2][0]
    items = [[(mono, 5, 0.3), (stereo, 40, 1.0)], [(stereo, 0, -1.0), (mono, -3, 3.7), (mono, 90, 1.0)], [(mono, 0, 1.0)]]
    got = _sum(k, items, 300, dtype=torch.float64).cpu().numpy()                  # channels: the largest among the files named
    assert got.shape == (3, 2, 300) and _same_bits(got, SR.restate(k.store, items, 300, 2))
    s = k.store.decode_window([stereo], [40], 300, dtype=torch.float64)[0].cpu().numpy()
    m = k.store.decode_window([mono], [5], 300, dtype=torch.float64)[0].cpu().numpy()
    assert m.shape == (1, 300) and m.any() and not np.array_equal(s[0], s[1])
    for c in range(2):
        assert _same_bits(got[0, c], (0.0 + 0.3 * m[0]) + 1.0 * s[c])
    assert _same_bits(got[2, 0], got[2, 1])
    assert _same_bits(got[2, 0], k.store.decode_window([mono], [0], 300, dtype=torch.float64)[0, 0].cpu().numpy())
    alone = _sum(k, [items[2]], 300, dtype=torch.float64)                         # mono files alone: one channel
    assert tuple(alone.shape) == (1, 1, 300) and _same_bits(alone.cpu().numpy()[0, 0], got[2, 0])
    out = torch.full((2, 1, 32), 12345, dtype=torch.int16, device=torch.device("cuda", 0))
    with pytest.raises(MrcError, match=r"mrc_pac_store_decode_window_sum: term 2: file %d is stereo" % stereo) as e:
        _sum(k, [[(mono, 0, 1.0), (mono, 9, 1.0)], [(stereo, 0, 1.0)]], 32, channels=1, out=out)
    assert e.value.code == -1 and bool((out == 12345).all())
    one = _sum(k, [[(mono, 0, 1.0), (mono, 9, 1.0)], [(stereo, 0, 1.0)]], 32, channels=1, out=out, mix="right")
    assert one is out and bool((out != 12345).any())


# ------------------------------------------------------------------ 5: independence
@pytest.mark.parametrize("D,mix,resample", [(1, None, None), (2, "mid", None), (2, None, (2, 3)), (1, "left", (160, 441))])
def test_result_depends_on_the_terms_order_and_on_nothing_else(kitchen, D, mix, resample):
    k = kitchen
    window = 300
    items = _items(k, D, resample, window, seed=4)
    kw = dict(channels=2 if mix is None else None, dtype=torch.float64, rate_divisor=D, mix=mix, resample=_rs(resample))
    base = _sum(k, items, window, **kw)
    assert k.store.stats()["slabs"] == 1
    assert _same(_sum(k, items[::-1], window, **kw).flip(0), base)                 # the items' order
    perm = np.random.default_rng(8).permutation(len(items))
    assert _same(_sum(k, [items[i] for i in perm], window, **kw), base[torch.from_numpy(perm).to(base.device)])
    for lo in range(0, len(items), 5):                           # split over several calls
        assert _same(_sum(k, items[lo:lo + 5], window, **kw), base[lo:lo + 5])
    for i in range(0, len(items), 7):
        assert _same(_sum(k, items[i:i + 1], window, **kw)[0], base[i])
    try:
        k.h.set_option(SLAB_OPTION, 1)                           # no two terms fit: every item is its own slab
        got = _sum(k, items, window, **kw)
        assert k.store.stats()["slabs"] == len(items) and _same(got, base)
        two = [items[2], items[2][::-1]] * 4                     # items of two terms: the rule counts the TERMS' spans
        assert len(items[2]) == 2
        span = window if resample is None else RS.span_bound(window, *resample, _w(resample))
        want = _sum(k, two, window, **kw)
        k.h.set_option(SLAB_OPTION, 4 * span)                    # two items of two terms per slab
        got = _sum(k, two, window, **kw)
        assert k.store.stats()["slabs"] == 4 and _same(got, want)
        k.h.set_option(SLAB_OPTION, 4 * span - 1)                # one term too many: an item per slab
        got = _sum(k, two, window, **kw)
        assert k.store.stats()["slabs"] == 8 and _same(got, want)
    finally:
        k.h.set_option(SLAB_OPTION, SLAB_DEFAULT)
    # the terms' order is part of the definition: reversed terms equal the restatement of the reversed terms
    rev = [it[::-1] for it in items]
    got = _sum(k, rev, window, **kw).cpu().numpy()
    assert _same_bits(got, SR.restate(k.store, rev, window, 2, D, mix, _rs(resample)))
    assert not _same_bits(got, base.cpu().numpy())               # ... and rounding makes them differ somewhere


def _w(resample):
    from mrcaudiocodec_amd.store import resample_taps
    return resample_taps(resample[0], resample[1], ZEROS, ROLLOFF)[0]


# ------------------------------------------------------------------ 6: work follows the windows
@pytest.mark.parametrize("D,mix,resample", [(1, None, None), (4, "mid", None), (2, "left", (2, 3))])
def test_chunks_parsed_are_the_sum_over_the_terms(kitchen, D, mix, resample):
    k = kitchen
    kw = dict(rate_divisor=D, mix=mix, resample=_rs(resample))
    cand = _candidates(k, D, resample, 300)
    past = cand[len(cand) // len(k.files) - 1]                   # the first file's start wholly past its end ...
    items = [[(f, s, g) for (f, s), g in zip(cand[0:3], (1.0, 0.0, -1.0))], [], [(past[0], past[1] + 10 * k.L, 1.0)],   # ... and its last block
             [(f, s, 0.0) for (f, s) in cand[3::5]]]
    alone, seen = [], set()
    for it in items:
        n = 0
        for (f, s, _) in it:
            k.store.decode_window([f], [s], 300, **kw)
            n += k.store.stats()["chunks_parsed"]
            seen.add(k.store.stats()["chunks_parsed"])
        alone.append(n)
    assert alone[1] == 0 and alone[2] == 0 and alone[0] > 0 and alone[3] > 0 and len(seen) > 2
    for it, n in zip(items, alone):
        _sum(k, [it], 300, **kw)
        st = k.store.stats()
        assert st["chunks_parsed"] == n and (st["decode_launches"] == 0) == (n == 0), (k.sid, it)
    _sum(k, items, 300, **kw)                                    # together: the sum (a zero gain is parsed like any other)
    st = k.store.stats()
    assert st["chunks_parsed"] == sum(alone) and st["slabs"] == 1 and st["ms"]["window_out"] > 0.0


# ------------------------------------------------------------------ 7: damage
@pytest.mark.parametrize("D,resample", [(1, None), (2, (2, 3))])
def test_damage_counts_only_inside_a_terms_span(kitchen, D, resample):
    from mrcaudiocodec_amd import MrcError
    from mrcaudiocodec_amd.store import PacStore
    k = kitchen
    ix, L = k.index[0], k.L
    j = int(ix["n_blocks"]) - 2                                   # the last joint block
    bad = bytearray(k.files[0])
    at = int(ix["chunk_offset"][j, 0]) + 4
    bad[at] = (bad[at] & 0x0F) | 0x40                             # table id 4
    up, down = resample or (1, 1)
    kw = dict(dtype=torch.float64, rate_divisor=D, resample=_rs(resample))
    with PacStore(k.h, [k.files[0], bytes(bad)]) as store:
        # windows over the file's first samples do not need block j: block i is needed iff p_i / D < last sample read + 1 + L / D
        w = 8
        last = (7 + w - 1) * down // up + (_w(resample) if resample else 0)
        assert int(ix["block_start"][j]) // D >= last + 1 + L // D
        files, starts = np.array([[0, 1], [1, 0]]), np.array([[7, 0], [3, -5]])
        gains = np.array([[1.0, 0.3], [-1.0, 3.7]])
        got = store.decode_window_sum(files, starts, gains, w, **kw)
        assert store.stats()["chunks_parsed"] > 0
        assert _same(got, k.store.decode_window_sum(np.zeros_like(files), starts, gains, w, **kw)) and bool(got.any())
        inside = ((int(ix["block_start"][j]) - L) // D) * up // down
        with pytest.raises(MrcError, match=r"mrc_pac_store_decode_window_sum: file 1: chunk at byte %d: %s"
                           % (at - 4, re.escape("table id not in {0..3, 15}"))) as e:
            store.decode_window_sum([[0, 1]], [[7, inside]], [[1.0, 0.0]], 3, **kw)     # (a zero gain is parsed like any other)
        assert e.value.code == -1
        assert bool(store.decode_window_sum([[0, 0]], [[7, inside]], [[1.0, 0.5]], 3, **kw).any())     # the sound file: no error


# ------------------------------------------------------------------ 8: the library's refusals
def _raw(k, D, mix, up, down, zeros, rolloff, offsets, files, starts, gains, window, channels, fmt=None, out="tensor", n_items=None):
    """the entry point itself -> (status, the pre-filled tensor)"""
    from mrcaudiocodec_amd import _lib
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)
    offsets, files, starts, gains = arr(offsets, np.int64), arr(files, np.int64), arr(starts, np.int64), arr(gains, np.float64)
    ptr = lambda a: None if a is None else a.ctypes.data
    n = (offsets.size - 1 if offsets is not None else 1) if n_items is None else n_items
    t = torch.full((max(n, 1), channels if channels in (1, 2) else 2, window if 0 < window <= 4096 else 16), 77, dtype=torch.float64,
                   device=torch.device("cuda", 0))
    rc = _lib.lib.mrc_pac_store_decode_window_sum(k.store._s, D, mix, up, down, zeros, rolloff, n, ptr(offsets), ptr(files), ptr(starts),
                                                  ptr(gains), window, channels, _lib.MRC_WINDOW_F64 if fmt is None else fmt,
                                                  t.data_ptr() if out == "tensor" else None, None)
    return rc, t


def test_library_refusals_come_before_any_device_work(kitchen):
    from mrcaudiocodec_amd import _lib
    k = kitchen
    E, MID = _lib.MRC_MIX_EACH, _lib.MRC_MIX_MID
    fn = "mrc_pac_store_decode_window_sum: "
    ok = dict(offsets=[0, 2], files=[0, 0], starts=[0, 9], gains=[1.0, 0.5], window=16, channels=2)
    head = dict(D=1, mix=E, up=1, down=1, zeros=16, rolloff=0.9)
    cases = [
        # the existing calls' refusals
        (dict(D=3), ("rate_divisor 3",)), (dict(D=0), ("rate_divisor 0",)), (dict(mix=7), ("mix 7", "MRC_MIX_EACH (3)")),
        (dict(mix=-1), ("mix -1",)), (dict(mix=MID), ("n_channels_out must be 1",)), (dict(channels=3), ("n_channels_out",)),
        (dict(channels=1), ("term 0: file 0 is stereo",)),
        (dict(up=1, down=9), ("down 9", "8 * up")), (dict(up=9, down=1), ("up 9", "8 * down")),
        (dict(up=1025, down=1024), ("up 1025",)), (dict(up=2, down=3, zeros=0), ("zeros 0",)),
        (dict(up=2, down=3, zeros=65), ("zeros 65",)), (dict(up=2, down=3, rolloff=0.25), ("rolloff",)),
        (dict(files=[0, len(k.files)]), ("file[1]", "outside the store")), (dict(files=[-1, 0]), ("file[0]", "outside the store")),
        (dict(window=-1), ("window",)), (dict(window=(1 << 40) + 1), ("window",)), (dict(fmt=9), ("format 9",)),
        (dict(out=None), ("out is NULL",)),
        # ... and this call's own
        (dict(up=0, down=3), ("up 0",)), (dict(up=2, down=0), ("down 0",)), (dict(up=-2, down=-2), ("up -2",)),
        (dict(offsets=None, n_items=1), ("term_offset is NULL",)), (dict(offsets=[1, 2]), ("term_offset[0] = 1",)),
        (dict(offsets=[0, 2, 1, 2], ), ("term_offset decreases at [2]",)), (dict(n_items=-1), ("n_items < 0",)),
        (dict(files=None), ("file, start or gain is NULL",)), (dict(starts=None), ("file, start or gain is NULL",)),
        (dict(gains=None), ("file, start or gain is NULL",)),
        (dict(gains=[1.0, float("nan")]), ("gain of term 1 is not finite",)),
        (dict(gains=[float("inf"), 1.0]), ("gain of term 0 is not finite",)),
        (dict(gains=[1.0, -float("inf")]), ("gain of term 1 is not finite",)),
    ]
    for change, words in cases:
        a = dict(head, **ok)
        a.update(change)
        rc, out = _raw(k, **a)
        text = _lib.lib.mrc_last_error(k.h._h).decode()
        assert rc == _lib.MRC_ERR_INVALID and bool((out == 77).all()), (change, rc, text)
        assert text.startswith(fn) and all(w in text for w in words), (change, text)
    # nothing to do: MRC_OK, nothing written
    for change in (dict(offsets=[0], files=None, starts=None, gains=None), dict(window=0), dict(offsets=[0], files=None, starts=None,
                                                                                                 gains=None, out=None)):
        rc, out = _raw(k, **dict(dict(head, **ok), **change))
        assert rc == 0 and bool((out == 77).all()), change
    # a ratio of 1 does not look at zeros and rolloff; items without terms need no term array
    rc, out = _raw(k, **dict(dict(head, **ok), up=7, down=7, zeros=0, rolloff=9.0))
    assert rc == 0 and bool((out != 77).all())
    rc, out = _raw(k, **dict(dict(head, **ok), offsets=[0, 0, 0], files=None, starts=None, gains=None))
    assert rc == 0 and not bool(out.any()) and not bool(torch.signbit(out).any())


def test_python_refusals_and_the_out_tensor(kitchen):
    k = kitchen
    dev = torch.device("cuda", 0)
    for bad in (torch.zeros((1, 2, 16), dtype=torch.float32, device=dev), torch.zeros((2, 2, 16), dtype=torch.float64, device=dev),
                torch.zeros((1, 2, 16), dtype=torch.float64), torch.zeros((1, 2, 32), dtype=torch.float64, device=dev)[:, :, ::2]):
        with pytest.raises(ValueError, match="decode_window_sum: out must be a contiguous"):
            k.store.decode_window_sum([[0, 0]], [[0, 5]], [[1.0, 1.0]], 16, channels=2, dtype=torch.float64, out=bad)
    out = torch.zeros((1, 2, 16), dtype=torch.float64, device=dev)
    assert k.store.decode_window_sum([[0, 0]], [[0, 5]], [[1.0, 1.0]], 16, out=out) is out and bool(out.any())
    assert tuple(k.store.decode_window_sum(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), 16).shape) == (0, 1, 16)
    assert tuple(k.store.decode_window_sum(np.zeros((4, 0)), np.zeros((4, 0)), np.zeros((4, 0)), 16).shape) == (4, 1, 16)
    assert tuple(k.store.decode_window_sum([[0]], [[0]], [[1.0]], 0).shape) == (1, 2, 0)


# ------------------------------------------------------------------ 9: the command line
def test_cli_overlays_at_an_snr(tmp_path, capsys):
    from mrcaudiocodec_amd import cli
    from mrcaudiocodec_amd.store import PacStore
    k = _kitchen_of("default")
    a, b, dst = str(tmp_path / "a.pac"), str(tmp_path / "b.pac"), str(tmp_path / "x.wav")
    for path in (a, b):                                          # (the one file at the default settings, under itself)
        with open(path, "wb") as fp:
            fp.write(k.files[0])
    rate = k.h.cfg.sample_rate
    n = int(k.index[0]["n_samples"])
    with PacStore(k.h, [k.files[0], k.files[0]]) as store:       # the store the command line builds
        g = float(store.levels().gains_for_snr(6.0, [0], [0], [1], [1500], n)[0])
        want = store.decode_window_sum([[0, 1]], [[0, 1500]], [[1.0, g]], n)[0].cpu().numpy()
        g2 = float(store.levels(2, "mid").gains_for_snr(-3.0, [0], [100], [1], [-40], 300)[0])
        want2 = store.decode_window_sum([[0, 1]], [[100, -40]], [[1.0, g2]], 300, rate_divisor=2, mix="mid")[0].cpu().numpy()
        g3 = float(store.levels(2, None).gains_for_snr(0.0, [0], [0], [1], [75], 450)[0])     # 300 samples at 16 kHz: 450 at 24 kHz
        want3 = store.decode_window_sum([[0, 1]], [[0, 50]], [[1.0, g3]], 300, rate_divisor=2, resample=(2, 3))[0].cpu().numpy()
    cli.main(["-d", a, dst, "--overlay", b, "--snr-db", "6", "--overlay-start", "1500"])
    assert open(dst, "rb").read() == cli.wav_bytes(want, rate) and want.shape == (2, n) and want.any()
    assert ("%.9g" % g) in capsys.readouterr().out and g != 1.0
    assert not np.array_equal(want, k.store.decode_window([0], [0], n)[0].cpu().numpy())
    # with an excerpt, a placement inside it, a mix and a rate divisor
    cli.main(["-d", a, dst, "--overlay", b, "--snr-db", "-3", "--overlay-start", "-40", "--start", "100", "--samples", "300",
              "--mix", "mid", "--rate-divisor", "2"])
    assert open(dst, "rb").read() == cli.wav_bytes(want2, rate // 2) and want2.shape == (1, 300) and want2.any()
    # at another sample rate
    cli.main(["-d", a, dst, "--overlay", b, "--snr-db", "0", "--overlay-start", "50", "--samples", "300", "--sample-rate", "16000"])
    assert open(dst, "rb").read() == cli.wav_bytes(want3, 16000) and want3.shape == (2, 300) and want3.any()
    # codec settings that differ are refused, the parameter named
    c = str(tmp_path / "c.pac")
    with open(c, "wb") as fp:
        fp.write(_kitchen_of("B").files[0])
    with pytest.raises(SystemExit):
        cli.main(["-d", a, dst, "--overlay", c, "--snr-db", "6"])
    assert "--overlay: n_mdct_lines differs" in capsys.readouterr().err


# ------------------------------------------------------------------ 10: linearity
def test_two_terms_are_a_plus_g_times_b(kitchen):
    k = kitchen
    window = 700
    cand = _candidates(k, 1, None, window)
    fa, sa = map(np.array, zip(*cand))
    fb, sb = fa[::-1].copy(), sa[::-1].copy()
    a = k.store.decode_window(fa, sa, window, channels=2, dtype=torch.float64).cpu().numpy()
    b = k.store.decode_window(fb, sb, window, channels=2, dtype=torch.float64).cpu().numpy()
    for g in (0.3, -0.3, 3.7, 1e-3):
        got = k.store.decode_window_sum(np.stack([fa, fb], 1), np.stack([sa, sb], 1), np.stack([np.ones(fa.size), np.full(fa.size, g)], 1),
                                        window, channels=2, dtype=torch.float64).cpu().numpy()
        want = a + g * b
        assert np.abs(got - want).max() <= 1e-12 and np.abs(want).max() > 1e-3
        pos = g * b >= 0
        assert pos.any() and np.array_equal(got[pos], want[pos])
