"""
GPU tests of the store's terms with spans and fades (mrc_pac_store_decode_window_spans, mrc_pac_store_stft_window_spans,
PacStore.decode_window_sum / stft_window(span_first=, span_len=, fade_in=, fade_out=)).

To the bit: the entries with all four arrays NULL against the reverb and STFT entries (bits and statistics); spans that cover
everything a call reads against the call without spans, in every format, with rooms, band gains, speeds and every STFT mode;
rows of abutting pieces against the concatenation of the existing one-term windows; every float64 row of dry terms against a
NumPy restatement -- the store's own EXISTING one-term float64 windows times the envelope in float64 (one division of two exact
integers, one product), folded by tests/sum_restatement.py -- over the windows, term counts, span places, span lengths and fades
at which the kernels' tile of 256 outputs, read-ahead of 4 terms and ramps can go wrong; independence of the rows' order, of
company and of the slab size.  Statistics: chunks_parsed is the sum of the existing one-term calls on the audible parts, empty
spans parse nothing, damage beside a span is not reported; the slab count follows the header's rule.
Within bounds: a crossfade of one file with itself (|row - v| <= 2^-51 |v|: two divisions, two products and one addition give
at most three units of 2^-53 to first order); convolved terms with partial spans within the reverb test's own bound of
np.convolve in longdouble of the restated d_k; STFT bins within the STFT test's bound of the long-double DFT of the spans
call's own float64 row, POWER and BANK to the bit from COMPLEX.
Files: those of tests/test_gpu_store_reduced.py at settings `default` and `B`; the bank: tests/store_rows_cases.py's responses
of 3 and 1500 taps.
"""
import re

import numpy as np
import pytest

import chain_kit as kit  # noqa: F401
from chain_kit import handles_closed_after_module  # noqa: F401
import reverb_reference as RV
import speed_restatement as SP
import stft_reference as SF
import store_rows_cases as RC
import sum_restatement as SR
from oracle import decode as odec
from test_store_span_cpu import envelope

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIDS = ("default", "B")
SLAB_OPTION, SLAB_DEFAULT = 7, 1 << 24
ROLLOFF, ZEROS = 0.9475, 16
WINDOWS = (1, 255, 256, 257, 700)                    # the tile of 256 outputs
TERM_COUNTS = (0, 1, 2, 4, 5, 9)                     # the read-ahead of 4 terms
LENS = (0, 1, 2, 256, 257, 5000)                     # span_len; the last: more than any window here
GAINS = (1.0, -1.0, 0.3, 3.7)
MIXES = (None, "mid", "left")
LISTS = {2: [(2, 3), (20, 27), (20, 33)],            # (tests/test_gpu_store_speed.py's lists of ratios)
         1: [(1, 1), (3, 2), (1, 3), (160, 441), (2, 3)],
         4: [(1, 1), (8, 1), (3, 2), (2, 3), (4, 5), (5, 4), (7, 8), (160, 147)]}
SINGLE = {"unit": [(1, 1)], "2/3": [(2, 3)], "3/2": [(3, 2)]}      # a list of one ratio: the single-ratio kernels
WIDE = (-(1 << 39), 1 << 40)                         # a span that covers every sample a call here can read
K_REVERB, N_REVERB = 8 * 0.32, 2048                  # tests/test_gpu_store_reverb.py: K and N = 2 REVERB_BLOCK
K_STFT = 8 * 2.13                                    # tests/test_gpu_store_stft.py: K = 17.04

_KITCHENS = {}


def _kitchen_of(sid):
    from test_gpu_store_reduced import _Kitchen
    if sid not in _KITCHENS:
        k = _Kitchen(sid)
        k.bank = RC.bank()
        k.store.set_impulse_responses(k.bank)
        _KITCHENS[sid] = k
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


def test_the_constants_are_the_other_tests():
    import test_gpu_store_reverb as TR
    import test_gpu_store_speed as TS
    import test_gpu_store_stft as TF
    assert (K_REVERB, N_REVERB, K_STFT) == (TR.K, TR.N_FFT, TF.K) and abs(K_STFT - 17.04) < 1e-12
    assert LISTS == TS.LISTS and WINDOWS == TS.WINDOWS and TERM_COUNTS == TS.TERM_COUNTS and (ZEROS, ROLLOFF) == (TS.ZEROS, TS.ROLLOFF)


# ------------------------------------------------------------------ rows of terms and their restatement
# a term: (file, start, gain, ratio index, ir, span_first, span_len, fade_in, fade_out)
def _ratio_kw(ratios):
    return dict(resample=(1, 1, ZEROS, ROLLOFF), speed_factors=[(down, up) for (up, down) in ratios])


def _flat(rows):
    terms = [t for row in rows for t in row]
    col = lambda j, t: np.array([v[j] for v in terms], dtype=t)
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return dict(files=col(0, np.int64), starts=col(1, np.int64), gains=col(2, np.float64), index=col(3, np.int32), irs=col(4, np.int32),
                first=col(5, np.int64), length=col(6, np.int64), fin=col(7, np.int64), fout=col(8, np.int64), offsets=offsets)


def _call(k, rows, window, ratios, spans=True, irs=False, store=None, **kw):
    a = _flat(rows)
    if spans:
        kw.update(span_first=a["first"], span_len=a["length"], fade_in=a["fin"], fade_out=a["fout"])
    if irs:
        kw.update(ir_index=a["irs"])
    return (store or k.store).decode_window_sum(a["files"], a["starts"], a["gains"], window, item_offsets=a["offsets"],
                                                speed_index=a["index"], **dict(_ratio_kw(ratios), **kw))


def _envelopes(a, lo, hi):
    """E [terms][hi - lo]: the envelope of every term at row samples lo <= t < hi, 0.0 where the term is silent"""
    E = np.zeros((len(a["files"]), hi - lo))
    for j in range(len(a["files"])):
        f, n = int(a["first"][j]), int(a["length"][j])
        t0, t1 = max(f, lo), min(f + n, hi)
        if t0 < t1:
            E[j, t0 - lo:t1 - lo] = envelope(n, int(a["fin"][j]), int(a["fout"][j]), t0 - f, t1 - f)
    return E


def _restate(k, rows, window, ratios, D=1, mix=None, **bands):
    """the float64 rows of dry terms: the EXISTING one-term windows times the envelope, folded in the terms' order"""
    a = _flat(rows)
    c = 1 if mix is not None else 2
    v = SP.term_windows(k.store, a["files"], a["starts"], a["index"], window, 2, ratios, ZEROS, ROLLOFF, D, mix, None, **bands)
    d = _envelopes(a, 0, window)[:, None, :] * v                     # (1.0 * v is v; 0.0 * v is a zero, which a fold from +0.0 cannot see)
    out = np.zeros((len(rows), c, window))
    for i in range(len(rows)):
        lo, hi = int(a["offsets"][i]), int(a["offsets"][i + 1])
        out[i] = SR.fold([d[j] for j in range(lo, hi)], a["gains"][lo:hi], (c, window))
    return out


def _fades(n, turn):
    """(fade_in, fade_out) for a span of n samples: none, one sample each, half each, and the two filling the span"""
    return [(0, 0), (min(1, n // 2), min(1, n // 2)), (n // 2, n // 2), (n // 3, n - n // 3), (n, 0), (0, n)][turn % 6]


def _rows(k, D, window, ratios, seed=0):
    """rows of TERM_COUNTS terms in turn: files, starts around block boundaries, ratios, span places and lengths and fades all
    cycling at different periods, until every (span_first, span_len) pair has been used"""
    firsts = (-300, -1, 0, 1, 255, 256, 257, window - 1, window, window + 5)
    rng = np.random.default_rng(seed)
    pairs = [(f, n) for f in firsts for n in LENS]
    order = rng.permutation(len(pairs))
    rows, at = [], 0
    while at < len(pairs):
        n_terms = TERM_COUNTS[len(rows) % len(TERM_COUNTS)]
        row = []
        for j in order[at:at + n_terms]:
            f = int(rng.integers(len(k.files)))
            r = int(rng.integers(len(ratios)))
            up, down = ratios[r]
            b = k.boundaries(f, D)
            start = int(b[int(rng.integers(len(b)))]) * up // down + int(rng.integers(-2, 3)) - int(rng.integers(0, window + 1))
            first, n = pairs[j]
            row.append((f, start, GAINS[int(j) % len(GAINS)], r, -1, first, n) + _fades(n, int(j)))
        rows.append(row)
        at += n_terms
    return rows


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _same(a, b):
    if a.dtype.is_complex:
        return a.dtype == b.dtype and _same(torch.view_as_real(a), torch.view_as_real(b))
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b) and \
        (not a.dtype.is_floating_point or torch.equal(torch.signbit(a), torch.signbit(b)))


def _stats(store):
    return {n: v for n, v in store.stats().items() if n != "ms"}


# ------------------------------------------------------------------ 1: all four arrays NULL: the reverb / STFT call itself
def _raw(k, name, values, out):
    """entry `name` with the header's arguments taken from values (arrays as RC.DTYPES types them, int64 for the span arrays) ->
    the status"""
    from mrcaudiocodec_amd import _lib
    held, args = [], []
    for a in kit.header_args(name):
        key = a.split()[-1].lstrip("*")
        v = k.store._s if key == "s" else out if key == "out" else values[key]
        if key in RAW_TYPES and v is not None:
            held.append(np.ascontiguousarray(v, dtype=RAW_TYPES[key]))
            v = held[-1].ctypes.data
        args.append(v)
    return int(getattr(_lib.lib, name)(*args))


RAW_TYPES = dict(RC.DTYPES, span_first=np.int64, span_len=np.int64, fade_in=np.int64, fade_out=np.int64)
RAW = dict(RC.DEFAULTS, n_items=2, term_offset=[0, 2, 3], file=[0, 0, 0], start=[5, 900, 64], gain=[1.0, 0.5, -2.0], ratio_of=[0, 1, 0],
           ir_of=[-1, 0, 1], window=300, n_frames=5, hop=40, n_fft=16, span_first=None, span_len=None, fade_in=None, fade_out=None)


@pytest.mark.parametrize("irs", [[-1, -1, -1], [-1, 0, 1]])
def test_null_spans_are_the_reverb_and_stft_calls(kitchen, irs):
    k = kitchen
    dev = torch.device("cuda", 0)
    values = dict(RAW, ir_of=irs)
    for new, old, shape in (("mrc_pac_store_decode_window_spans", "mrc_pac_store_decode_window_reverb", (2, 2, 300)),
                            ("mrc_pac_store_stft_window_spans", "mrc_pac_store_stft_window", (2, 2, 9, 5))):
        got, want = torch.full(shape, 77.0, dtype=torch.float64, device=dev), torch.full(shape, 77.0, dtype=torch.float64, device=dev)
        assert _raw(k, old, values, want.data_ptr()) == 0
        st_want = _stats(k.store)
        assert _raw(k, new, values, got.data_ptr()) == 0
        assert _stats(k.store) == st_want and st_want["chunks_parsed"] > 0
        assert _same(got, want) and bool((got != 77.0).all()) and bool(got.any())


# ------------------------------------------------------------------ 2: spans that cover everything are the call without spans
def _wide(rows):
    return [[t[:5] + WIDE + (0, 0) for t in row] for row in rows]


@pytest.mark.parametrize("mix", MIXES)
@pytest.mark.parametrize("D", sorted(LISTS))
def test_spans_over_everything_change_no_bit_of_dry_rows(kitchen, D, mix):
    k = kitchen
    kw = dict(channels=2 if mix is None else None, mix=mix, rate_divisor=D)
    for window in (257, 700):
        rows = _wide(_rows(k, D, window, LISTS[D], seed=window))
        for dtype in (torch.float64, torch.float32, torch.int16):
            want = _call(k, rows, window, LISTS[D], spans=False, dtype=dtype, **kw)
            st = _stats(k.store)
            got = _call(k, rows, window, LISTS[D], dtype=dtype, **kw)
            assert _same(got, want) and bool(got.any()), (k.sid, D, mix, window, dtype)
            assert _stats(k.store)["chunks_parsed"] == st["chunks_parsed"]


@pytest.mark.parametrize("name", sorted(SINGLE))
def test_spans_over_everything_change_no_bit_with_rooms_band_gains_and_one_ratio(kitchen, name):
    from mrcaudiocodec_amd.store import critical_band_edges
    k = kitchen
    ratios, window = SINGLE[name], 700
    rows = _wide(_rows(k, 1, window, ratios, seed=3))
    n_terms = sum(len(r) for r in rows)
    rows = [[t[:4] + ((i + j) % 3 - 1,) + t[5:] for j, t in enumerate(row)] for i, row in enumerate(rows)]      # dry, 3 taps, 1500 taps
    n_bands = critical_band_edges(k.h.cfg.sample_rate).size - 1
    bg = np.random.default_rng(5).uniform(0.0, 2.0, (n_terms, n_bands))
    for kw in (dict(channels=2), dict(mix="mid", band_gains=bg)):
        for dtype in (torch.float64, torch.int16):
            want = _call(k, rows, window, ratios, spans=False, irs=True, dtype=dtype, **kw)
            got = _call(k, rows, window, ratios, irs=True, dtype=dtype, **kw)
            assert _same(got, want) and bool(got.any()), (k.sid, name, sorted(kw), dtype)


@pytest.mark.parametrize("output", ["complex", "power", "bank"])
def test_spans_over_everything_change_no_bit_of_any_stft_mode(kitchen, output):
    k = kitchen
    n_fft, hop, n_frames = 16, 40, 5
    rows = _wide(_rows(k, 2, 300, LISTS[2], seed=8))[:12]
    rows = [[t[:4] + ((i + j) % 3 - 1,) + t[5:] for j, t in enumerate(row)] for i, row in enumerate(rows)]
    a = _flat(rows)
    kw = dict(gains=a["gains"], item_offsets=a["offsets"], speed_index=a["index"], ir_index=a["irs"], rate_divisor=2, mix="mid",
              output=output, dtype=torch.float64, frame_window=RC.FRAME_WINDOW, bank=RC.BANK_MATRIX if output == "bank" else None,
              resample=(2, 3, ZEROS, ROLLOFF), speed_factors=[(1, 1), (9, 10), (11, 10)])
    for center in (False, True):                                     # (centred: starts and spans move together)
        want = k.store.stft_window(a["files"], a["starts"], n_frames, hop, n_fft, center=center, **kw)
        got = k.store.stft_window(a["files"], a["starts"], n_frames, hop, n_fft, center=center, span_first=a["first"], span_len=a["length"], **kw)
        assert _same(got, want) and bool(torch.view_as_real(got).any() if got.is_complex() else got.any()), (k.sid, output, center)


# ------------------------------------------------------------------ 3: abutting pieces are a concatenation
@pytest.mark.parametrize("D,mix,ratio", [(1, None, (1, 1)), (2, "mid", (2, 3)), (1, "left", (3, 2)), (4, None, (160, 147))])
def test_abutting_pieces_are_the_concatenation_of_the_existing_windows(kitchen, D, mix, ratio):
    from mrcaudiocodec_amd.store import concat_spans
    k = kitchen
    rng = np.random.default_rng(D)
    up, down = ratio
    rs = {} if up == down else dict(resample=(up, down, ZEROS, ROLLOFF))
    kw = dict(channels=2 if mix is None else None, mix=mix, rate_divisor=D)
    for window, K in ((700, 8), (257, 5), (256, 1), (9, 9)):
        cuts = np.sort(rng.choice(np.arange(1, window), K - 1, replace=False)) if K > 1 else np.zeros(0, np.int64)
        lengths = np.diff(np.concatenate([[0], cuts, [window]])).astype(np.int64)[None, :].repeat(3, 0)
        files = rng.integers(0, len(k.files), (3, K))
        src = np.array([[int(rng.choice(k.boundaries(int(f), D))) * up // down + int(rng.integers(-3, 4)) for f in row] for row in files])
        starts, first, length, fin, fout = concat_spans(lengths, src)
        assert not fin.any() and not fout.any() and np.array_equal(first[:, 0], np.zeros(3)) and np.all(first[:, -1] + length[:, -1] == window)
        for dtype in (torch.float64, torch.float32, torch.int16):
            got = k.store.decode_window_sum(files, starts, np.ones((3, K)), window, dtype=dtype, span_first=first, span_len=length,
                                            speed_factors=[(down, up)], speed_index=np.zeros((3, K), np.int32),
                                            resample=(1, 1, ZEROS, ROLLOFF), **kw).cpu().numpy()
            for i in range(3):
                pieces = [k.store.decode_window([int(files[i, j])], [int(src[i, j])], int(lengths[i, j]), dtype=dtype, **dict(kw, **rs))[0].cpu().numpy()
                          for j in range(K)]
                assert _same_bits(got[i], np.concatenate(pieces, axis=-1)), (k.sid, D, mix, ratio, window, dtype, i)
            assert np.abs(got.astype(np.float64)).max() > 0


# ------------------------------------------------------------------ 4: every float64 row of dry terms is the restatement
@pytest.mark.parametrize("mix", MIXES)
@pytest.mark.parametrize("D", sorted(LISTS))
def test_rows_of_terms_with_spans_and_fades_equal_the_restatement(kitchen, D, mix):
    k = kitchen
    for window in WINDOWS:
        rows = _rows(k, D, window, LISTS[D], seed=window)
        assert {len(r) for r in rows[:-1]} == set(TERM_COUNTS)
        got = _call(k, rows, window, LISTS[D], channels=2 if mix is None else None, dtype=torch.float64, mix=mix, rate_divisor=D).cpu().numpy()
        want = _restate(k, rows, window, LISTS[D], D, mix)
        assert got.shape == (len(rows), 2 if mix is None else 1, window)
        assert _same_bits(got, want), (k.sid, D, mix, window, np.abs(got - want).max(), np.argwhere(got != want)[:4].tolist())
        if window > 1:
            assert np.abs(got).max() > 1e-3 and not _same_bits(got, _restate(k, _wide(rows), window, LISTS[D], D, mix))


@pytest.mark.parametrize("name", sorted(SINGLE))
@pytest.mark.parametrize("D", [1, 2])
def test_rows_at_one_ratio_equal_the_restatement_with_and_without_band_gains(kitchen, D, name):
    from mrcaudiocodec_amd.store import critical_band_edges
    k = kitchen
    ratios = SINGLE[name]
    n_bands = critical_band_edges(k.h.cfg.sample_rate).size - 1
    for window in WINDOWS:
        rows = _rows(k, D, window, ratios, seed=window + 7)
        bg = np.random.default_rng(window).uniform(-1.5, 1.5, (sum(len(r) for r in rows), n_bands))
        for bands in ({}, dict(band_gains=bg)):
            got = _call(k, rows, window, ratios, channels=2, dtype=torch.float64, rate_divisor=D, **bands).cpu().numpy()
            want = _restate(k, rows, window, ratios, D, None, **bands)
            assert _same_bits(got, want), (k.sid, D, name, window, bool(bands), np.abs(got - want).max())
    f64 = _call(k, rows, 700, ratios, channels=2, dtype=torch.float64, rate_divisor=D).cpu().numpy()
    assert np.array_equal(_call(k, rows, 700, ratios, channels=2, rate_divisor=D).cpu().numpy(), odec.pcm16(f64))
    assert np.array_equal(_call(k, rows, 700, ratios, channels=2, dtype=torch.float32, rate_divisor=D).cpu().numpy(), f64.astype(np.float32))


# ------------------------------------------------------------------ 5: independence
@pytest.mark.parametrize("D,mix,irs", [(2, None, False), (1, "mid", False), (4, None, False), (1, None, True)])
def test_result_depends_on_the_terms_order_and_on_nothing_else(kitchen, D, mix, irs):
    k = kitchen
    window = 300
    rows = _rows(k, D, window, LISTS[D], seed=4)
    if irs:                                                          # convolved terms with partial spans: equal to the bit all the same
        rows = [[t[:4] + ((i + j) % 3 - 1,) + t[5:] for j, t in enumerate(row)] for i, row in enumerate(rows)]
    kw = dict(channels=2 if mix is None else None, dtype=torch.float64, mix=mix, rate_divisor=D, irs=irs)
    base = _call(k, rows, window, LISTS[D], **kw)
    assert k.store.stats()["slabs"] == 1 and bool(base.any())
    perm = np.random.default_rng(8).permutation(len(rows))
    assert _same(_call(k, [rows[i] for i in perm], window, LISTS[D], **kw), base[torch.from_numpy(perm).to(base.device)])
    for i in range(0, len(rows), 4):                                 # alone, and in other company
        assert _same(_call(k, rows[i:i + 1], window, LISTS[D], **kw)[0], base[i])
        assert _same(_call(k, rows[i:i + 3], window, LISTS[D], **kw), base[i:i + 3])
    try:
        k.h.set_option(SLAB_OPTION, 1)                               # every row is its own slab
        got = _call(k, rows, window, LISTS[D], **kw)
        assert k.store.stats()["slabs"] >= len(rows) and _same(got, base)
    finally:
        k.h.set_option(SLAB_OPTION, SLAB_DEFAULT)
    if not irs:
        rev = [row[::-1] for row in rows]                            # the terms' order is part of the definition
        got = _call(k, rev, window, LISTS[D], **kw).cpu().numpy()
        assert _same_bits(got, _restate(k, rev, window, LISTS[D], D, mix))
        # ... and where three terms sound at once rounding makes the two orders differ somewhere (two terms commute)
        three = [[(0, 40 + 9 * j, g, j % len(LISTS[D]), -1, 10, 200, 50, 60) for j, g in enumerate((0.3, 3.7, -1.0))]]
        fwd, bwd = (_call(k, r, window, LISTS[D], **kw).cpu().numpy() for r in (three, [three[0][::-1]]))
        assert _same_bits(fwd, _restate(k, three, window, LISTS[D], D, mix)) and not _same_bits(fwd, bwd)
        assert np.abs(fwd - bwd).max() <= 1e-12 and not fwd[:, :, :10].any() and not fwd[:, :, 210:].any()


# ------------------------------------------------------------------ 6: work follows the spans; damage
def _audible(t, window):
    return max(t[5], 0), min(t[5] + t[6], window)


@pytest.mark.parametrize("D,mix", [(2, None), (1, "left"), (4, "mid")])
def test_chunks_parsed_are_those_of_the_one_term_calls_on_the_audible_parts(kitchen, D, mix):
    k = kitchen
    window = 700
    rows = _rows(k, D, window, LISTS[D], seed=2)[:12]
    total = 0
    for t in (t for row in rows for t in row):
        a0, a1 = _audible(t, window)
        if a0 < a1:
            up, down = LISTS[D][t[3]]
            rs = {} if up == down else dict(resample=(up, down, ZEROS, ROLLOFF))
            k.store.decode_window([t[0]], [t[1] + a0], a1 - a0, rate_divisor=D, mix=mix, **rs)
            total += k.store.stats()["chunks_parsed"]
    _call(k, rows, window, LISTS[D], channels=2 if mix is None else None, mix=mix, rate_divisor=D)
    st = k.store.stats()
    assert st["chunks_parsed"] == total > 0 and st["slabs"] == 1
    _call(k, _wide(rows), window, LISTS[D], channels=2 if mix is None else None, mix=mix, rate_divisor=D)
    assert k.store.stats()["chunks_parsed"] > total                 # (the same terms heard over the whole row need more)
    # spans that are all empty -- no sample, wholly before the row, wholly behind it -- parse nothing and give +0.0
    silent = [[t[:5] + s + (0, 0) for t, s in zip(row, [(5, 0), (-300, 300), (window, 9), (window + 5, 1 << 40)] * 3)] for row in rows]
    got = _call(k, silent, window, LISTS[D], channels=2 if mix is None else None, mix=mix, rate_divisor=D, dtype=torch.float64)
    st = k.store.stats()
    assert st["chunks_parsed"] == 0 and st["decode_launches"] == 0 and not bool(got.any()) and not bool(torch.signbit(got).any())


def test_damage_counts_only_inside_a_terms_span(kitchen):
    from mrcaudiocodec_amd import MrcError
    from mrcaudiocodec_amd.store import PacStore
    k = kitchen
    ix, L = k.index[0], k.L
    j = int(ix["n_blocks"]) - 2                                       # the last joint block (the speed test's damage)
    bad = bytearray(k.files[0])
    at = int(ix["chunk_offset"][j, 0]) + 4
    bad[at] = (bad[at] & 0x0F) | 0x40                                 # table id 4
    with PacStore(k.h, [k.files[0], bytes(bad)]) as store:
        for D, ratios in ((1, [(1, 1)]), (2, [(2, 3), (20, 33)])):
            for r, (up, down) in enumerate(ratios):
                W = 0 if up == down else 2 * ZEROS * 8               # (more than any half width here)
                inside = ((int(ix["block_start"][j]) - L) // D) * up // down      # in the damaged block, in this ratio's output samples
                window = inside + 3
                quiet = max(0, min(64, ((int(ix["block_start"][j]) - 2 * L) // D - W) * up // down - 8))
                assert quiet > 0
                row = lambda f, first, n: [[(0, 7, 1.0, 0, -1, 0, window, 0, 0), (f, 0, 0.5, r, -1, first, n, 1, 1)]]
                # the window covers the damaged block, the span does not: not read, not reported, the sound file's bits
                got = _call(k, row(1, 2, quiet), window, ratios, store=store, dtype=torch.float64, rate_divisor=D)
                assert store.stats()["chunks_parsed"] > 0
                assert _same(got, _call(k, row(0, 2, quiet), window, ratios, dtype=torch.float64, rate_divisor=D)) and bool(got.any())
                with pytest.raises(MrcError, match=r"mrc_pac_store_decode_window_spans: file 1: chunk at byte %d: %s"
                                   % (at - 4, re.escape("table id not in {0..3, 15}"))) as e:
                    _call(k, row(1, inside, 3), window, ratios, store=store, dtype=torch.float64, rate_divisor=D)
                assert e.value.code == -1
                assert bool(_call(k, row(0, inside, 3), window, ratios, store=store, dtype=torch.float64, rate_divisor=D).any())


# ------------------------------------------------------------------ 7: slabs
def _plane_span(t, window, ratios, half_widths):
    a0, a1 = _audible(t, window)
    if a0 >= a1:
        return 0
    up, down = ratios[t[3]]
    return a1 - a0 if up == down else -(-(a1 - a0 - 1) * down // up) + 2 * half_widths[t[3]]


def _slabs(rows, span, limit):
    """the header's rule: runs of whole rows whose terms, each counted at span, sum to at most limit (one row at least)"""
    n, first = 0, 0
    while first < len(rows):
        last, terms = first + 1, len(rows[first])
        while last < len(rows) and (terms + len(rows[last])) * span <= limit:
            terms += len(rows[last])
            last += 1
        n, first = n + 1, last
    return n


@pytest.mark.parametrize("D", [1, 2])
def test_slabs_follow_the_longest_span_and_change_no_bit(kitchen, D):
    from mrcaudiocodec_amd.store import resample_taps
    k = kitchen
    ratios, window = LISTS[D][:3], 700
    W = [0 if up == down else resample_taps(up, down, ZEROS, ROLLOFF)[0] for (up, down) in ratios]
    # eight abutting pieces of window / 8 + remainder per row, rows of 8 terms: about one window per row, not eight
    rows = [[(i % len(k.files), 100 * i + 87 * j, 1.0, (i + j) % 3, -1, 87 * j, 87 if j < 7 else window - 609, 0, 0) for j in range(8)]
            for i in range(9)]
    span = max(_plane_span(t, window, ratios, W) for row in rows for t in row)
    assert 0 < span < window                                          # (a term counts at its piece's span, not at the window)
    kw = dict(channels=2, dtype=torch.float64, rate_divisor=D)
    base = _call(k, rows, window, ratios, **kw)
    assert k.store.stats()["slabs"] == 1 and bool(base.any())
    try:
        for limit in (8 * span - 1, 8 * span, 16 * span, 24 * span - 1, 72 * span):
            k.h.set_option(SLAB_OPTION, limit)
            got = _call(k, rows, window, ratios, **kw)
            assert k.store.stats()["slabs"] == _slabs(rows, span, limit), (limit, span)
            assert _same(got, base)
        assert [_slabs(rows, span, v * span) for v in (8, 16, 72)] == [9, 5, 1] and _slabs(rows, span, 8 * span - 1) == 9
    finally:
        k.h.set_option(SLAB_OPTION, SLAB_DEFAULT)


# ------------------------------------------------------------------ 8: a crossfade of a file with itself
@pytest.mark.parametrize("F", [1, 7, 160])
def test_a_crossfade_of_a_signal_with_itself_is_the_signal(kitchen, F):
    k = kitchen
    window, at = 700, 257
    for name in sorted(SINGLE):
        ratios = SINGLE[name]
        rows = [[(f, 300, 1.0, 0, -1, 0, at + F, 0, F), (f, 300, 1.0, 0, -1, at, window - at, F, 0)] for f in range(len(k.files))]
        got = _call(k, rows, window, ratios, channels=2, dtype=torch.float64).cpu().numpy()
        v = _call(k, _wide([row[:1] for row in rows]), window, ratios, channels=2, dtype=torch.float64).cpu().numpy()
        assert np.abs(v[:, :, at:at + F]).max() > 1e-4
        worst = float((np.abs(got - v) / np.where(v == 0, 1.0, np.abs(v))).max()) / 2.0 ** -53
        print("crossfade of %d samples at %s: |row - v| at most %.3g units of 2^-53 |v|" % (F, name, worst))
        assert np.all(np.abs(got - v) <= 2.0 ** -51 * np.abs(v)), (k.sid, F, name, worst)
        assert _same_bits(got[:, :, :at], v[:, :, :at]) and _same_bits(got[:, :, at + F:], v[:, :, at + F:])     # no product outside the ramps
        assert _same_bits(got, _restate(k, rows, window, ratios))


# ------------------------------------------------------------------ 9: convolved terms with partial spans
@pytest.mark.parametrize("window", [257, 1025])
def test_convolved_terms_with_partial_spans_meet_the_reverb_bound(kitchen, window):
    k = kitchen
    ratios = LISTS[1][:2]
    lpre = len(k.bank[1]) - 1
    spans = [(-lpre - 5, lpre + 60), (-700, 690), (-1, 2), (0, window), (100, 50), (window - 1, 9), (window, 5), (40, 0), (-2000, 400)]
    rows, t = [], 0
    for i in range(len(spans)):
        row = []
        for j in range(TERM_COUNTS[1 + i % 5]):
            f, n = spans[t % len(spans)]
            row.append((t % len(k.files), 200 + 37 * t, GAINS[t % 4], t % 2, (t % 3) - 1, f, n) + _fades(n, t))
            t += 1
        rows.append(row)
    got = _call(k, rows, window, ratios, irs=True, channels=2, dtype=torch.float64).cpu().numpy()
    a = _flat(rows)
    dry = SP.term_windows(k.store, a["files"], a["starts"] - lpre, a["index"], window + lpre, 2, ratios, ZEROS, ROLLOFF)
    d = _envelopes(a, -lpre, window)[:, None, :] * dry               # the restated d_k over [-Lpre, window)
    ref, unit = np.zeros((len(rows), 2, window), np.longdouble), np.zeros(len(rows))
    for i in range(len(rows)):
        for j in range(a["offsets"][i], a["offsets"][i + 1]):
            h = np.array([1.0]) if a["irs"][j] < 0 else k.bank[a["irs"][j]]
            w = d[j][:, lpre - (len(h) - 1):]
            for c in range(2):
                ref[i, c] += np.longdouble(a["gains"][j]) * RV.wet_reference(h, w[c])
            unit[i] += abs(a["gains"][j]) * RV.error_scale(h, w, N_REVERB)
    err = np.abs(got.astype(np.longdouble) - ref).reshape(len(rows), -1).max(axis=1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        excess = np.where(unit > 0, err / (K_REVERB * unit), np.where(err > 0, np.inf, 0.0))
    print("window %d: convolved terms with partial spans, largest error %.3g of the reverb bound (K = %g)" % (window, excess.max(), K_REVERB))
    assert np.all(excess <= 1.0), (window, excess.tolist())
    assert np.abs(got).max() > 1e-3 and np.abs(ref[:, :, -1]).max() > 0          # (a gated piece rings on to the row's end)
    wide = _call(k, _wide(rows), window, ratios, irs=True, channels=2, dtype=torch.float64).cpu().numpy()
    assert np.abs(wide - got).max() > 1e-3                            # (the spans did something)


# ------------------------------------------------------------------ 10: the STFT of rows with partial spans
@pytest.mark.parametrize("n_fft,hop,n_frames", [(16, 5, 7), (400, 160, 3)])
def test_stft_of_rows_with_partial_spans(kitchen, n_fft, hop, n_frames):
    from mrcaudiocodec_amd.store import hann_window
    k = kitchen
    L = (n_frames - 1) * hop + n_fft
    g = hann_window(n_fft) * (1.0 + 0.5 * np.arange(n_fft) / n_fft) + 0.01
    ratios = LISTS[1][:2]
    rows = _rows(k, 1, L, ratios, seed=n_fft)[:10]
    rows = [[t[:4] + ((i + j) % 3 - 1,) + t[5:] for j, t in enumerate(row)] for i, row in enumerate(rows)]
    a = _flat(rows)
    kw = dict(gains=a["gains"], item_offsets=a["offsets"], speed_index=a["index"], ir_index=a["irs"], channels=2, frame_window=g,
              span_first=a["first"], span_len=a["length"], fade_in=a["fin"], fade_out=a["fout"], dtype=torch.float64, **_ratio_kw(ratios))
    x = _call(k, rows, L, ratios, irs=True, channels=2, dtype=torch.float64).cpu().numpy()     # the spans call's own float64 row
    z = k.store.stft_window(a["files"], a["starts"], n_frames, hop, n_fft, output="complex", **kw).cpu().numpy()
    gx = (SF.frames_of(x, n_fft, hop, n_frames) * g).reshape(-1, n_fft)
    re, im = SF.dft(gx)
    zz = np.moveaxis(z, 2, 3).reshape(-1, n_fft // 2 + 1)
    err = SF.ratio(zz.real, zz.imag, re, im, SF.unit(gx))
    print("n_fft %d: STFT of rows with partial spans, largest error %.3g of the bound (K = %g)" % (n_fft, err / K_STFT, K_STFT))
    assert err <= K_STFT and np.abs(x).max() > 1e-3
    p = k.store.stft_window(a["files"], a["starts"], n_frames, hop, n_fft, output="power", **kw).cpu().numpy()
    assert np.array_equal(p, z.real * z.real + z.imag * z.imag) and p.max() > 0
    bank = np.random.default_rng(1).uniform(0.0, 1.0, (3, n_fft // 2 + 1)) * (np.arange(n_fft // 2 + 1) % 4 != 0)
    bank[1, :3] = 0.0
    e = k.store.stft_window(a["files"], a["starts"], n_frames, hop, n_fft, output="bank", bank=bank, **kw).cpu().numpy()
    want = np.zeros(p.shape[:2] + (3, n_frames))
    for q, row in enumerate(bank):
        nz = np.flatnonzero(row)
        for kk in range(nz[0], nz[-1] + 1):
            want[:, :, q] = want[:, :, q] + row[kk] * p[:, :, kk]
    assert np.array_equal(e, want) and e.max() > 0


# ------------------------------------------------------------------ 11: the library's refusals, word for word
REFUSALS = [
    (dict(span_first=[0, 0, 0]), "span_first is given without span_len"),
    (dict(span_len=[4, 4, 4]), "span_len is given without span_first"),
    (dict(fade_in=[0, 0, 0]), "fade_in is given without spans (span_first and span_len)"),
    (dict(fade_out=[0, 0, 0]), "fade_out is given without spans (span_first and span_len)"),
    (dict(span_first=[0, 0, 0], span_len=[4, -1, 4]), "span_len of term 1 = -1 is outside [0, 2^40]"),
    (dict(span_first=[0, 0, 0], span_len=[4, 4, (1 << 40) + 1]), "span_len of term 2 = 1099511627777 is outside [0, 2^40]"),
    (dict(span_first=[(1 << 40) + 1, 0, 0], span_len=[4, 4, 4]), "span_first of term 0 = 1099511627777 is outside [-2^40, 2^40]"),
    (dict(span_first=[0, -(1 << 40) - 1, 0], span_len=[4, 4, 4]), "span_first of term 1 = -1099511627777 is outside [-2^40, 2^40]"),
    (dict(span_first=[0, 0, 0], span_len=[4, 4, 4], fade_in=[0, -1, 0]), "fade_in of term 1 = -1 is negative"),
    (dict(span_first=[0, 0, 0], span_len=[4, 4, 4], fade_out=[0, 0, -7]), "fade_out of term 2 = -7 is negative"),
    (dict(span_first=[0, 0, 0], span_len=[4, 4, 4], fade_in=[3, 0, 0], fade_out=[2, 0, 0]),
     "fade_in + fade_out of term 0 = 3 + 2 exceeds its span_len = 4"),
    (dict(span_first=[0, 0, 0], span_len=[4, 0, 4], fade_out=[0, 1, 0]), "fade_in + fade_out of term 1 = 0 + 1 exceeds its span_len = 0"),
    # ... and the underlying entry's own, under the new name
    (dict(mix=7), "mix 7 is not MRC_MIX_EACH (3), MRC_MIX_MID (0), MRC_MIX_LEFT (1) or MRC_MIX_RIGHT (2)"),
    (dict(ir_of=[0, 5, 0]), "ir_of of term 1 = 5 is neither -1 nor inside the bank of 2 impulse responses"),
    (dict(gain=[1.0, float("nan"), 1.0]), "gain of term 1 is not finite"),
    (dict(file=[0, 99, 0]), None),
]


def test_library_refusals_name_the_argument_and_leave_out_untouched(kitchen):
    from mrcaudiocodec_amd import _lib
    k = kitchen
    out = torch.full((4096,), 77.0, dtype=torch.float64, device=torch.device("cuda", 0))
    for name in ("mrc_pac_store_decode_window_spans", "mrc_pac_store_stft_window_spans"):
        for change, text in REFUSALS:
            rc = _raw(k, name, dict(RAW, **change), out.data_ptr())
            got = _lib.lib.mrc_last_error(k.h._h).decode()
            assert rc == _lib.MRC_ERR_INVALID and bool((out == 77.0).all()), (name, change, rc, got)
            if text is None:
                assert got.startswith(name + ": file[1] = 99 is outside the store's"), got
            else:
                assert got == name + ": " + text, (name, change, got)
        # fade_in + fade_out == span_len is allowed, an empty span too; the call as it stands writes every value
        ok = dict(RAW, span_first=[0, -5, 9], span_len=[4, 0, 6], fade_in=[1, 0, 6], fade_out=[3, 0, 0])
        assert _raw(k, name, ok, out.data_ptr()) == 0 and not bool((out[:180] == 77.0).any())
        out.fill_(77.0)
    # the refusals that need a length the call itself forms: window -1 (decode), n_fft 22 (stft) come under the new names too
    assert _raw(k, "mrc_pac_store_decode_window_spans", dict(RAW, window=-1), out.data_ptr()) == _lib.MRC_ERR_INVALID
    assert _lib.lib.mrc_last_error(k.h._h).decode() == "mrc_pac_store_decode_window_spans: window must lie in [0, 2^40]"
    assert _raw(k, "mrc_pac_store_stft_window_spans", dict(RAW, n_fft=22), out.data_ptr()) == _lib.MRC_ERR_INVALID
    assert _lib.lib.mrc_last_error(k.h._h).decode().startswith("mrc_pac_store_stft_window_spans: n_fft 22 must be even")
    assert bool((out == 77.0).all())


# ------------------------------------------------------------------ 12: the command line
def test_cli_appends_a_file_with_a_crossfade(tmp_path, capsys):
    from mrcaudiocodec_amd import cli
    from mrcaudiocodec_amd.store import PacStore, concat_spans
    k = _kitchen_of("default")
    a, b, dst = str(tmp_path / "a.pac"), str(tmp_path / "b.pac"), str(tmp_path / "x.wav")
    for path in (a, b):
        with open(path, "wb") as fp:
            fp.write(k.files[0])
    with PacStore(k.h, [k.files[0], k.files[0]]) as store:
        n = int(store.n_samples_resampled(2, 3, 2)[0])
        for fade, flags in ((0, []), (160, ["--crossfade", "160"])):
            starts, first, length, fin, fout = concat_spans([[n, n]], [[0, 0]], crossfade=fade)
            want = store.decode_window_sum([[0, 1]], starts, [[1.0, 1.0]], 2 * n - fade, rate_divisor=2, mix="mid", resample=(2, 3),
                                           span_first=first, span_len=length, fade_in=fin, fade_out=fout)[0].cpu().numpy()
            one = store.decode_window([0], [0], n, rate_divisor=2, mix="mid", resample=(2, 3))[0].cpu().numpy()
            assert np.array_equal(want[:, :n - fade], one[:, :n - fade]) and np.array_equal(want[:, n:], one[:, fade:]) and one.any()
            cli.main(["-d", a, dst, "--append", b, "--sample-rate", "16000", "--mix", "mid"] + flags)
            assert open(dst, "rb").read() == cli.wav_bytes(want, 16000) and want.shape == (1, 2 * n - fade)
            assert "1 channels x %d samples" % (2 * n - fade) in capsys.readouterr().out
    for argv, text in ((["a.pac", "x.wav", "--append", "b.pac"], "it needs -d"), (["-d", "a.pac", "x.wav", "--crossfade", "3"], "it needs --append"),
                       (["-d", "a.pac", "x.wav", "--append", "b.pac", "--crossfade", "-1"], "not a whole number of samples >= 0"),
                       (["-d", "a.pac", "x.wav", "--append", "b.pac", "--speed", "11/10"], "it does not take --speed")):
        with pytest.raises(SystemExit):
            cli.main(argv)
        assert text in capsys.readouterr().err
