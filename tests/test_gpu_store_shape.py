"""
GPU tests of the store's band gains on the MDCT lines (mrc_pac_store_decode_window_shaped, PacStore.decode_window(band_gains=),
PacStore.decode_window_sum(band_gains=), cli -d --band-gains-db): gains of 1.0 are the existing calls bit for bit in all three
formats; gains that are all one power of two are decode_window_sum at that term gain, bit for bit; per-item gains in [-2, 2] on
edges that do not match the codec's bands against the NumPy restatement on the lines (tests/shape_restatement.py) to 1e-12 of
the file's peak times max(1, max |gain|) -- the bar tests/test_gpu_decode.py, the reduced-rate and the mix tests hold an
inverse transform to, scaled by the gain; the other formats as conversions of the call's own float64 window; rows of terms as
the left fold over the one-term shaped windows; independence of order, company, slab size and how a window is cut, the gain
rows following their items; the chunks parsed; the library's refusals; the command line.  Files: tests/mix_restatement.files.
Everything oracle-side is computed once per module and never written to.
"""
import numpy as np
import pytest

import chain_kit as kit  # noqa: F401
from chain_kit import handles_closed_after_module  # noqa: F401
import mix_restatement as MR
import shape_restatement as SH
import sum_restatement as SR
from oracle import decode as odec

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIDS = MR.KIT_SIDS + ("default",)
SLAB_OPTION, SLAB_DEFAULT = 7, 1 << 24
FORMATS = (torch.int16, torch.float32, torch.float64)
MIXES = (None, "mid", "left", "right")
FN = "mrc_pac_store_decode_window_shaped"

_KITCHENS = {}


def _kitchen(sid):
    from test_gpu_store_mix import _Kitchen
    if sid not in _KITCHENS:
        k = _Kitchen(sid)
        k.rate = int(k.h.cfg.sample_rate)
        k.blocks = {}
        _KITCHENS[sid] = k
    return _KITCHENS[sid]


@pytest.fixture(scope="module", params=SIDS)
def kitchen(request):
    return _kitchen(request.param)


@pytest.fixture(scope="module", autouse=True)
def stores_closed_after_module():
    yield
    for k in _KITCHENS.values():
        k.store.close()
    _KITCHENS.clear()


def _odd_edges(k):
    """edges that do not match the codec's bands: edge[0] > 0, the last edge below Nyquist (and above the Nyquist of D = 2 and
    4), and one band between two neighbouring line centres of a short block, which holds no line of such a block"""
    sp = k.rate / (2.0 * k.S)
    f2 = 2.5 * sp
    return np.array(sorted([0.0065 * k.rate, f2 + 0.1 * sp, f2 + 0.4 * sp, 0.07 * k.rate, 0.11 * k.rate, 0.2 * k.rate, 0.31 * k.rate]))


def _rows(n, n_bands, seed):
    """distinct rows in [-2, 2] with exact zeros and sign flips among them; row 0: all zeros, row 1: all ones"""
    g = np.random.default_rng(seed).uniform(-2.0, 2.0, (n, n_bands))
    for i in range(n):
        g[i, i % n_bands] = 0.0
        g[i, (i + 3) % n_bands] = -g[i, (i + 2) % n_bands]
    g[0], g[1 % n] = 0.0, 1.0
    return g


def _kw(mix):
    return dict(channels=2 if mix is None else None, mix=mix)


def _same(a, b):
    return torch.equal(a, b) and (a.dtype == torch.int16 or torch.equal(torch.signbit(a), torch.signbit(b)))


def _cut(ref, start, window):
    out = np.zeros(ref.shape[:-1] + (window,), ref.dtype)
    lo, hi = max(start, 0), min(start + window, ref.shape[-1])
    if hi > lo:
        out[..., lo - start:hi - start] = ref[..., lo:hi]
    return out


# ------------------------------------------------------------------ 1: gains of 1.0 are the existing calls
@pytest.mark.parametrize("D", MR.DIVISORS)
def test_ones_are_the_existing_call_bit_for_bit(kitchen, D):
    k = kitchen
    files, starts = map(np.array, zip(*k.items(D)))
    window = 3 * k.S // D + 5
    for edges in (None, _odd_edges(k)):
        ones = np.ones((files.size, 25 if edges is None else edges.size - 1))
        for mix in MIXES:
            for dtype in FORMATS:
                want = k.store.decode_window(files, starts, window, dtype=dtype, rate_divisor=D, **_kw(mix))
                got = k.store.decode_window(files, starts, window, dtype=dtype, rate_divisor=D, band_gains=ones, band_edges_hz=edges,
                                            **_kw(mix))
                assert got.dtype == dtype and _same(got, want) and bool(want.any()), (k.sid, D, mix, dtype)
                if dtype != torch.int16:
                    assert not bool(torch.signbit(got)[got == 0].any())
    # one row for every item
    got = k.store.decode_window(files, starts, window, dtype=torch.float64, rate_divisor=D, band_gains=np.ones(25), **_kw(None))
    assert _same(got, k.store.decode_window(files, starts, window, dtype=torch.float64, rate_divisor=D, **_kw(None)))


@pytest.mark.parametrize("mix", (None, "mid"))
def test_ones_under_resample_and_in_sums(mix):
    k = _kitchen("default")
    D, rs, window = 2, (2, 3), 300
    files, starts = map(np.array, zip(*[(f, s * 2 // 3) for f, s in k.items(D)]))
    ones = np.ones((files.size, 25))
    for dtype in FORMATS:
        want = k.store.decode_window(files, starts, window, dtype=dtype, rate_divisor=D, resample=rs, **_kw(mix))
        got = k.store.decode_window(files, starts, window, dtype=dtype, rate_divisor=D, resample=rs, band_gains=ones, **_kw(mix))
        assert _same(got, want) and bool(want.any())
    # rows of K = 2 terms
    n = files.size // 2
    f2, s2 = files[:2 * n].reshape(n, 2), starts[:2 * n].reshape(n, 2)
    g2 = np.random.default_rng(1).uniform(-2, 2, (n, 2))
    for kw in (dict(rate_divisor=1), dict(rate_divisor=D, resample=rs)):
        for dtype in FORMATS:
            want = k.store.decode_window_sum(f2, s2, g2, window, dtype=dtype, **kw, **_kw(mix))
            got = k.store.decode_window_sum(f2, s2, g2, window, dtype=dtype, band_gains=np.ones((n, 2, 25)), **kw, **_kw(mix))
            assert _same(got, want) and bool(want.any())


# ------------------------------------------------------------------ 2: one power of two on every band
@pytest.mark.parametrize("D", MR.DIVISORS)
def test_a_power_of_two_on_every_band_is_that_term_gain(kitchen, D):
    k = kitchen
    files, starts = map(np.array, zip(*k.items(D)))
    window = k.L // D + 3
    edges = np.array([0.0, 0.013 * k.rate, 0.2 * k.rate, k.rate / 2.0])          # [0, Nyquist]: every line in a band
    for mix in (None, "mid"):
        for g in (0.25, -2.0):
            got = k.store.decode_window(files, starts, window, dtype=torch.float64, rate_divisor=D, band_gains=np.full(3, g),
                                        band_edges_hz=edges, **_kw(mix))
            want = k.store.decode_window_sum(files[:, None], starts[:, None], np.full((files.size, 1), g), window, dtype=torch.float64,
                                             rate_divisor=D, **_kw(mix))
            assert torch.equal(got, want) and bool(want.any()), (k.sid, D, mix, g)


# ------------------------------------------------------------------ 3: per-item gains against the restatement on the lines
def _blocks(k, f, mid):
    if (f, mid) not in k.blocks:
        k.blocks[(f, mid)] = SH.blocks(k.files[f], k.S, k.blksw, mid and k.nch[f] == 2)
    return k.blocks[(f, mid)]


def _restatement_is_a_reference(k, f, mid, D):
    """whether the NumPy restatement of file f lies within 1e-12 of the file's peak of the exact evaluation of the same
    (unshaped) lines: only then can it hold anything to that bar.  Decided on the CPU, from the oracle alone, once."""
    key = ("own", f, mid, D)
    if key not in k.blocks:
        planes, blks = _blocks(k, f, mid)
        one = (k.rate, [0.0, k.rate / 2.0], [1.0])
        own = np.abs(SH.synthesise(planes, blks, D, *one) - SH.synthesise_exact(planes, blks, D, *one))[:, k.L // D:].max()
        k.blocks[key] = float(own) / np.abs(k.ref(f, D)).max()
        print("%s file %d%s D = %d: the NumPy restatement lies %.3g of the file's peak from the exact evaluation"
              % (k.sid, f, " (mid)" if mid else "", D, k.blocks[key]))
    return k.blocks[key] <= 1e-12


@pytest.mark.parametrize("D", MR.DIVISORS)
def test_f64_equals_the_restatement_on_the_lines(kitchen, D):
    """Every file of the kit, whole, under rows of gains of its own, against tests/shape_restatement.py at
    1e-12 x the file's peak x max(1, max |gain|).
    The NumPy restatement is the reference wherever it is one at that bar: wherever its own distance from the exact evaluation
    of the same lines (shape_restatement.synthesise_exact: the transform's definition in long double, no code under test) is
    within 1e-12 of the file's peak.  That holds for every file and D of the kit but one: setting K's one-block mono file at
    D = 1, where oracle.decode.IMDCT itself lies 1.64e-12 of the file's peak from the exact transform (4.7e-14 absolute, the
    size it has on the setting's other files, whose peak is 0.41; the store keeps the second half of that lone block, where
    its aliasing mostly cancels, so the file's peak, 0.029, is 14 times below the amplitude inside the transform, which the
    reference's rounded phase 2 pi n0 k / N follows).  There the exact evaluation, rounded to float64, stands in its place,
    at the same bar; nothing is left out.
    Measured on an MI355X against the NumPy restatement, worst over files, rows and mixes, as a fraction of the file's peak (bar
    2e-12, max |gain| being 1.995): B 4.4e-13 / 2.4e-13 / 1.2e-13 at D = 1 / 2 / 4, C 6.1e-14 / 4.6e-14 / 2.6e-14,
    D 2.8e-13 / 3.2e-13 / 1.5e-13, K 5.0e-13 / 2.1e-13 at D = 2 / 4, default 2.0e-13 / 5.7e-14 / 3.6e-14; K's one-block mono
    file at D = 1 against NumPy: 2.17e-12, the reference's own error times the gain."""
    k = kitchen
    edges = _odd_edges(k)
    nb = edges.size - 1
    short = SH.line_bands(k.rate, k.S, k.S, edges)
    assert any(not (short == q).any() for q in range(nb)) and (short == SH.NO_BAND).any()      # a band without a short line
    assert edges[0] > 0 and k.rate / 8 < edges[-1] < k.rate / 2
    margin = 2 * k.L // D + 7
    n_max = max(int(ix["n_samples"]) for ix in k.index) // D
    window = n_max + 2 * margin
    files = np.repeat(np.arange(len(k.files)), max(2, -(-6 // len(k.files))))    # every file under two rows or more; neighbours differ
    starts = np.full(files.size, -margin)
    rows = _rows(files.size, nb, seed=len(k.files))
    assert len({tuple(r) for r in rows}) == files.size and (rows < 0).any() and (rows == 0).any() and np.abs(rows).max() <= 2.0
    bar = max(1.0, np.abs(rows).max())
    plain = k.store.decode_window(files, starts, window, dtype=torch.float64, rate_divisor=D, **_kw(None)).cpu().numpy()
    worst, exact = 0.0, set()
    for mix in MIXES:
        got = k.store.decode_window(files, starts, window, dtype=torch.float64, rate_divisor=D, band_gains=rows, band_edges_hz=edges,
                                    **_kw(mix)).cpu().numpy()
        assert got.shape == (files.size, 2 if mix is None else 1, window)
        for i, f in enumerate(files):
            planes, blks = _blocks(k, f, mix == "mid")
            if _restatement_is_a_reference(k, f, mix == "mid", D):
                ref = SH.synthesise(planes, blks, D, k.rate, edges, rows[i])[:, k.L // D:]
            else:
                ref = SH.synthesise_exact(planes, blks, D, k.rate, edges, rows[i])[:, k.L // D:].astype(np.float64)
                exact.add(int(f))
            n = ref.shape[1]
            assert n == int(k.index[f]["n_samples"]) // D
            if mix in ("left", "right"):
                ref = ref[min(MIXES.index(mix) - 2, planes - 1)][None]
            elif mix is None and planes == 1:
                ref = np.concatenate([ref, ref])                     # a mono file fills both channels
            peak = np.abs(k.ref(f, D)).max()
            err = np.abs(got[i][:, margin:margin + n] - ref).max() / peak
            worst = max(worst, err)
            assert err <= 1e-12 * bar, (k.sid, D, mix, f, i, err)
            outside = np.concatenate([got[i][:, :margin], got[i][:, margin + n:]], axis=1)
            assert not outside.any() and not np.signbit(outside).any()
            if i == 0:
                # row 0, every in-band gain zero: what is left is the lines outside every band, unchanged -- and it is signal
                assert np.abs(ref).max() > 1e-6 * peak and not np.array_equal(got[i], plain[i][:got.shape[1]])
    print("%s D = %d: worst max |delta| = %.3g of the peak (bar %.3g); files held to the exact evaluation: %s"
          % (k.sid, D, worst, 1e-12 * bar, sorted(exact) or "none"))
    assert len(exact) <= 1 and (not exact or len(k.files) > 1)      # the NumPy restatement stays the reference for all but one file


# ------------------------------------------------------------------ 4: the other formats
@pytest.mark.parametrize("D,mix", [(1, None), (2, "mid"), (4, "left")])
def test_formats_are_conversions_of_the_f64_window(kitchen, D, mix):
    k = kitchen
    files, starts = map(np.array, zip(*k.items(D)))
    window = 3 * k.S // D + 5
    edges = _odd_edges(k)
    rows = _rows(files.size, edges.size - 1, seed=2) * 4.0         # (up to 8: some windows pass full scale and saturate)
    kw = dict(rate_divisor=D, band_gains=rows, band_edges_hz=edges, **_kw(mix))
    f64 = k.store.decode_window(files, starts, window, dtype=torch.float64, **kw).cpu().numpy()
    i16 = k.store.decode_window(files, starts, window, **kw)
    f32 = k.store.decode_window(files, starts, window, dtype=torch.float32, **kw)
    assert i16.dtype == torch.int16 and f32.dtype == torch.float32 and f64.any()
    assert np.array_equal(i16.cpu().numpy(), odec.pcm16(f64))
    assert np.array_equal(f32.cpu().numpy(), f64.astype(np.float32))


# ------------------------------------------------------------------ 5: rows of terms
@pytest.mark.parametrize("D,mix,resample", [(1, None, None), (2, "mid", None), (2, None, (2, 3)), (1, "left", (160, 441))])
def test_rows_of_terms_are_the_fold_over_the_one_term_shaped_windows(kitchen, D, mix, resample):
    k = kitchen
    up, down = resample or (1, 1)
    cand = [(f, s * up // down) for f, s in k.items(D)]
    order = np.random.default_rng(3).permutation(len(cand))
    window = 300
    edges = _odd_edges(k)
    files, starts = map(np.array, zip(*[cand[j] for j in order]))
    n = files.size
    rows = _rows(n, edges.size - 1, seed=5)
    gains = np.random.default_rng(6).uniform(-2, 2, n)
    offsets = [0]
    while offsets[-1] < n:                                           # rows of two and three terms in turn
        offsets.append(min(n, offsets[-1] + (2 if len(offsets) % 2 else 3)))
    offsets = np.array(offsets)
    kw = dict(dtype=torch.float64, rate_divisor=D, resample=resample, band_edges_hz=edges, **_kw(mix))
    got = k.store.decode_window_sum(files, starts, gains, window, item_offsets=offsets, band_gains=rows, **kw).cpu().numpy()
    one = k.store.decode_window(files, starts, window, band_gains=rows, **kw).cpu().numpy()
    assert {int(v) for v in np.diff(offsets)} >= {2, 3} and got.shape == (offsets.size - 1,) + one.shape[1:] and got.any()
    for i in range(offsets.size - 1):
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        want = SR.fold([one[j] for j in range(lo, hi)], gains[lo:hi])
        assert np.array_equal(got[i], want), (k.sid, D, mix, resample, i)
    # ... and the rows matter: the same call with the terms' rows swapped differs
    swapped = k.store.decode_window_sum(files, starts, gains, window, item_offsets=offsets, band_gains=rows[::-1].copy(), **kw)
    assert not np.array_equal(swapped.cpu().numpy(), got)


# ------------------------------------------------------------------ 6: independence
@pytest.mark.parametrize("D,mix", [(1, None), (2, "mid"), (4, "right")])
def test_result_depends_on_the_items_and_their_rows_alone(kitchen, D, mix):
    k = kitchen
    files, starts = map(np.array, zip(*k.items(D)))
    n, window = files.size, 2 * k.S // D + 9
    edges = _odd_edges(k)
    rows = _rows(n, edges.size - 1, seed=7)                          # neighbouring items: different rows
    kw = dict(dtype=torch.float64, rate_divisor=D, band_edges_hz=edges, **_kw(mix))
    call = lambda sel, **more: k.store.decode_window(files[sel], starts[sel], window, band_gains=rows[sel], **dict(kw, **more))
    every = np.arange(n)
    base = call(every)
    assert k.store.stats()["slabs"] == 1 and bool(base.any())
    perm = np.random.default_rng(8).permutation(n)
    assert _same(call(perm), base[torch.from_numpy(perm).to(base.device)])
    assert _same(call(every[::-1].copy()).flip(0), base)
    for lo in range(0, n, 7):                                        # other company
        assert _same(call(every[lo:lo + 7]), base[lo:lo + 7])
    for i in range(0, n, 11):
        assert _same(call(every[i:i + 1])[0], base[i])
    try:
        k.h.set_option(SLAB_OPTION, 1)                               # every item its own slab
        got = call(every)
        assert k.store.stats()["slabs"] == n and _same(got, base)
        k.h.set_option(SLAB_OPTION, 3 * window)                      # three items per slab: the rows follow their items
        got = call(every)
        assert k.store.stats()["slabs"] == -(-n // 3) and _same(got, base)
    finally:
        k.h.set_option(SLAB_OPTION, SLAB_DEFAULT)
    cut = window // 2 + 1                                            # a window cut in two
    first = k.store.decode_window(files, starts, cut, band_gains=rows, **kw)
    second = k.store.decode_window(files, starts + cut, window - cut, band_gains=rows, **kw)
    assert _same(torch.cat([first, second], dim=2), base)


# ------------------------------------------------------------------ 7: work follows the windows
@pytest.mark.parametrize("D,mix", [(1, None), (2, "mid"), (4, "left")])
def test_chunks_parsed_are_the_unshaped_calls(kitchen, D, mix):
    k = kitchen
    files, starts = map(np.array, zip(*k.items(D)))
    window = k.S // D + 1
    k.store.decode_window(files, starts, window, rate_divisor=D, **_kw(mix))
    want = k.store.stats()
    k.store.decode_window(files, starts, window, rate_divisor=D, band_gains=np.full(25, 0.5), **_kw(mix))
    got = k.store.stats()
    assert got["chunks_parsed"] == want["chunks_parsed"] > 0 and got["decode_launches"] == want["decode_launches"]
    assert got["slabs"] == want["slabs"] == 1 and got["plan_bytes_uploaded"] > want["plan_bytes_uploaded"]


# ------------------------------------------------------------------ 8: the library's refusals
def _raw(k, D, mix, up, down, zeros, rolloff, n_bands, edges, band_gains, offsets, files, starts, gains, window, channels, fmt=None,
         out="tensor", n_items=None):
    """the entry point itself -> (status, the pre-filled tensor)"""
    from mrcaudiocodec_amd import _lib
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)
    offsets, files, starts = arr(offsets, np.int64), arr(files, np.int64), arr(starts, np.int64)
    gains, edges, band_gains = arr(gains, np.float64), arr(edges, np.float64), arr(band_gains, np.float64)
    ptr = lambda a: None if a is None else a.ctypes.data
    n = (offsets.size - 1 if offsets is not None else 1) if n_items is None else n_items
    t = torch.full((max(n, 1), channels if channels in (1, 2) else 2, window if 0 < window <= 4096 else 16), 77, dtype=torch.float64,
                   device=torch.device("cuda", 0))
    rc = _lib.lib.mrc_pac_store_decode_window_shaped(k.store._s, D, mix, up, down, zeros, rolloff, n_bands, ptr(edges), ptr(band_gains), n,
                                                     ptr(offsets), ptr(files), ptr(starts), ptr(gains), window, channels,
                                                     _lib.MRC_WINDOW_F64 if fmt is None else fmt,
                                                     t.data_ptr() if out == "tensor" else None, None)
    return rc, t


def test_library_refusals_come_before_any_device_work(kitchen):
    from mrcaudiocodec_amd import _lib
    k = kitchen
    E, MID = _lib.MRC_MIX_EACH, _lib.MRC_MIX_MID
    nan, inf = float("nan"), float("inf")
    ok = dict(D=1, mix=E, up=1, down=1, zeros=16, rolloff=0.9, n_bands=2, edges=[0.0, 1000.0, 5000.0], band_gains=[[1.0, 0.5], [0.0, -1.0]],
              offsets=[0, 2], files=[0, 0], starts=[0, 9], gains=[1.0, 0.5], window=16, channels=2)
    cases = [
        # this call's own
        (dict(n_bands=0), ("n_bands 0", "1..256")), (dict(n_bands=257), ("n_bands 257", "1..256")), (dict(n_bands=-1), ("n_bands -1",)),
        (dict(edges=[0.0, 5000.0, 1000.0]), ("edge_hz is not strictly increasing at [2]",)),
        (dict(edges=[0.0, 1000.0, 1000.0]), ("edge_hz is not strictly increasing at [2]",)),
        (dict(edges=[-1.0, 1000.0, 5000.0]), ("edge_hz[0] < 0",)), (dict(edges=[0.0, nan, 5000.0]), ("edge_hz[1] is not finite",)),
        (dict(edges=[0.0, 1000.0, inf]), ("edge_hz[2] is not finite",)),
        (dict(edges=None), ("edge_hz or band_gain is NULL",)), (dict(band_gains=None), ("edge_hz or band_gain is NULL",)),
        (dict(band_gains=[[1.0, 0.5], [0.0, nan]]), ("band_gain of term 1, band 1 is not finite",)),
        (dict(band_gains=[[1.0, inf], [0.0, 1.0]]), ("band_gain of term 0, band 1 is not finite",)),
        (dict(band_gains=[[1.0, 1.0], [-inf, 1.0]]), ("band_gain of term 1, band 0 is not finite",)),
        # every refusal class of the sum call
        (dict(D=3), ("rate_divisor 3",)), (dict(mix=7), ("mix 7", "MRC_MIX_EACH (3)")), (dict(mix=MID), ("n_channels_out must be 1",)),
        (dict(channels=3), ("n_channels_out",)), (dict(channels=1), ("term 0: file 0 is stereo",)),
        (dict(up=1, down=9), ("down 9", "8 * up")), (dict(up=2, down=3, zeros=0), ("zeros 0",)),
        (dict(up=2, down=3, rolloff=0.25), ("rolloff",)), (dict(up=0, down=3), ("up 0",)),
        (dict(files=[0, len(k.files)]), ("file[1]", "outside the store")), (dict(window=-1), ("window",)), (dict(fmt=9), ("format 9",)),
        (dict(out=None), ("out is NULL",)),
        (dict(offsets=None, n_items=1), ("term_offset is NULL",)), (dict(offsets=[1, 2]), ("term_offset[0] = 1",)),
        (dict(offsets=[0, 2, 1, 2]), ("term_offset decreases at [2]",)), (dict(n_items=-1), ("n_items < 0",)),
        (dict(files=None), ("file, start or gain is NULL",)), (dict(gains=None), ("file, start or gain is NULL",)),
        (dict(gains=[1.0, nan]), ("gain of term 1 is not finite",)),
    ]
    for change, words in cases:
        a = dict(ok)
        a.update(change)
        rc, out = _raw(k, **a)
        text = _lib.lib.mrc_last_error(k.h._h).decode()
        assert rc == _lib.MRC_ERR_INVALID and bool((out == 77).all()), (change, rc, text)
        assert text.startswith(FN + ": ") and all(w in text for w in words), (change, text)
    # the call as it stands is accepted and equals the Python front; nothing to do: MRC_OK, nothing written
    rc, out = _raw(k, **ok)
    want = k.store.decode_window_sum([[0, 0]], [[0, 9]], [[1.0, 0.5]], 16, channels=2, dtype=torch.float64,
                                     band_gains=[ok["band_gains"]], band_edges_hz=ok["edges"])
    assert rc == 0 and _same(out, want) and bool(out.any())
    for change in (dict(window=0), dict(offsets=[0], files=None, starts=None, gains=None, edges=None, band_gains=None)):
        rc, out = _raw(k, **dict(ok, **change))
        assert rc == 0 and bool((out == 77).all()), change


# ------------------------------------------------------------------ 9: the command line
def test_cli_band_gains_db(tmp_path, capsys):
    from mrcaudiocodec_amd import cli
    from mrcaudiocodec_amd.store import PacStore, gains_from_db
    k = _kitchen("default")
    a, b, dst = str(tmp_path / "a.pac"), str(tmp_path / "b.pac"), str(tmp_path / "x.wav")
    for path in (a, b):
        with open(path, "wb") as fp:
            fp.write(k.files[0])
    n = int(k.index[0]["n_samples"])
    spec = "0-300:-inf,3400-9000:-6,9000-24000:-inf"
    edges, gains = [0.0, 300.0, 3400.0, 9000.0, 24000.0], gains_from_db([-np.inf, 0.0, -6.0, -np.inf])
    with PacStore(k.h, [k.files[0], k.files[0]]) as store:           # the store the command line builds
        kw = dict(band_gains=gains, band_edges_hz=edges)
        want = store.decode_window([0], [0], n, **kw)[0].cpu().numpy()
        plain = store.decode_window([0], [0], n)[0].cpu().numpy()
        want2 = store.decode_window([0], [100], 300, rate_divisor=2, mix="mid", **kw)[0].cpu().numpy()
        want3 = store.decode_window([0], [0], 300, rate_divisor=2, resample=(2, 3), **kw)[0].cpu().numpy()
        g = float(store.levels().gains_for_snr(6.0, [0], [0], [1], [1500], n)[0])
        want4 = store.decode_window_sum([[0, 1]], [[0, 1500]], [[1.0, g]], n, band_edges_hz=edges,
                                        band_gains=[[gains, np.ones(4)]])[0].cpu().numpy()
    cli.main(["-d", a, dst, "--band-gains-db", spec])
    assert open(dst, "rb").read() == cli.wav_bytes(want, k.rate) and want.shape == (2, n) and want.any()
    assert not np.array_equal(want, plain)
    cli.main(["-d", a, dst, "--band-gains-db", spec, "--mix", "mid", "--rate-divisor", "2", "--start", "100", "--samples", "300"])
    assert open(dst, "rb").read() == cli.wav_bytes(want2, k.rate // 2) and want2.shape == (1, 300) and want2.any()
    cli.main(["-d", a, dst, "--band-gains-db", spec, "--sample-rate", "16000", "--samples", "300"])
    assert open(dst, "rb").read() == cli.wav_bytes(want3, 16000) and want3.shape == (2, 300) and want3.any()
    cli.main(["-d", a, dst, "--band-gains-db", spec, "--overlay", b, "--snr-db", "6", "--overlay-start", "1500"])
    assert open(dst, "rb").read() == cli.wav_bytes(want4, k.rate) and want4.any() and not np.array_equal(want4, want)
    assert ("%.9g" % g) in capsys.readouterr().out
