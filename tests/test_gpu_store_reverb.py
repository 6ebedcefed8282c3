"""
GPU tests of the store's reverberated windows (mrc_pac_store_set_irs, mrc_pac_store_decode_window_reverb,
PacStore.set_impulse_responses / decode_window(ir_index=) / decode_window_sum(ir_index=), cli -d --ir).

Accuracy.  The reference of a convolved term is np.convolve in np.longdouble (tests/reverb_reference.py) of the store's own
EXISTING float64 window at (start - Lpre, window + Lpre) -- the code this call is built around, not the code under test --
and a row is folded in longdouble.  The allowed error per output is
    K * 2^-52 * log2(N) * sum over the row's terms of |gain| * sum|h| * max|w|        (N = 2 * REVERB_BLOCK = 2048),
max|w| over the dry window's channels (a stereo term's channels share one complex transform) and an unconvolved term counted
as the response [1.0] (its product and the fold's additions round in float64 too).  K is 8 times the largest error that
NumPy's own float64 FFT convolution shows against the same reference on the cases of test_convolved_terms_meet_the_bound, in
the same unit: that ratio was measured as NUMPY_RATIO below (the test measures it again and holds it to the record), which
leaves room for another factorisation and for the additions of the partitions.
Everything else is equality to the bit: unconvolved rows against the existing calls, independence of order, company, slab
size and the bank's layout, repeated calls, the format conversions, decode_window(ir_index=) against a one-term row.
Files: those of tests/test_gpu_store_reduced.py (settings `default` and `B`).
"""
import numpy as np
import pytest

import chain_kit as kit  # noqa: F401
from chain_kit import handles_closed_after_module  # noqa: F401
import reverb_reference as RV
from oracle import codec as ocodec, decode as odec, pacfile as opac

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIDS = ("default", "B")
SLAB_OPTION, SLAB_DEFAULT = 7, 1 << 24
B = 1024                                             # MRC_STORE_REVERB_BLOCK (asserted below)
N_FFT = 2 * B
NUMPY_RATIO = 0.32                                   # NumPy's FFT convolution: its largest error in units of error_scale (0.318 measured)
K = 8 * NUMPY_RATIO
LENGTHS = RV.bank_lengths(B)                         # 1, 2, B - 1, B, B + 1, 2 B, 2 B + 1, 3 B + 17
WINDOWS = (1, 255, 257, B - 1, B, B + 1, 2 * B + 1)
ZEROS, ROLLOFF = 16, 0.9475
SPEEDS = dict(resample=(2, 3, ZEROS, ROLLOFF), speed_factors=[(1, 1), (9, 10), (11, 10)])

_KITCHENS = {}


def _kitchen_of(sid):
    from test_gpu_store_reduced import _Kitchen
    if sid not in _KITCHENS:
        k = _Kitchen(sid)
        k.bank = [RV.room(n, 100 + n) for n in LENGTHS]
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


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b) and \
        (not a.dtype.is_floating_point or torch.equal(torch.signbit(a), torch.signbit(b)))


def _flat(rows):
    """rows of (file, start, gain, ir) -> files, starts, gains, irs, offsets"""
    terms = [t for row in rows for t in row]
    col = lambda j, t: np.array([v[j] for v in terms], dtype=t)
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return col(0, np.int64), col(1, np.int64), col(2, np.float64), col(3, np.int32), offsets


def _call(k, rows, window, store=None, bank_map=None, **kw):
    files, starts, gains, irs, offsets = _flat(rows)
    if bank_map is not None:
        irs = np.array([bank_map[i] if i >= 0 else -1 for i in irs], np.int32)
    return (store or k.store).decode_window_sum(files, starts, gains, window, item_offsets=offsets, ir_index=irs, **kw)


def _existing(k, files, starts, window, store=None, **kw):
    """the EXISTING float64 windows of single terms, one-term rows at gain 1.0 -> numpy [terms][channels][window]"""
    n = len(files)
    return (store or k.store).decode_window_sum(np.asarray(files, np.int64), np.asarray(starts, np.int64), np.ones(n), window,
                                                item_offsets=np.arange(n + 1), dtype=torch.float64, **kw).cpu().numpy()


def _reference(k, rows, window, bank=None, store=None, **kw):
    """-> (the rows in longdouble [rows][channels][window], the allowed error without K [rows], NumPy's largest ratio)"""
    bank = k.bank if bank is None else bank
    files, starts, gains, irs, offsets = _flat(rows)
    lpre = max([len(bank[i]) for i in irs if i >= 0], default=1) - 1
    dry = _existing(k, files, starts - lpre, window + lpre, store=store, **kw) if len(files) else np.zeros((0, 1, window + lpre))
    channels = dry.shape[1] if len(files) else (1 if kw.get("mix") else kw.get("channels", 2))
    ref = np.zeros((len(rows), channels, window), np.longdouble)
    unit = np.zeros(len(rows))
    worst = 0.0
    for r in range(len(rows)):
        for j in range(offsets[r], offsets[r + 1]):
            h = np.array([1.0]) if irs[j] < 0 else bank[irs[j]]
            w = dry[j][:, lpre - (len(h) - 1):]
            for c in range(channels):
                ref[r, c] += np.longdouble(gains[j]) * RV.wet_reference(h, w[c])
                if irs[j] >= 0:
                    worst = max(worst, RV.numpy_ratio(h, w[c], N_FFT))
            unit[r] += abs(gains[j]) * RV.error_scale(h, w, N_FFT)
    return ref, unit, worst


def _excess(got, ref, unit):
    """the largest |got - ref| per row in units of the row's allowed error K * unit (rows that allow none: 0 if exact, else inf)"""
    err = np.abs(got.astype(np.longdouble) - ref).reshape(len(ref), -1).max(axis=1).astype(np.float64) if ref.size else np.zeros(len(ref))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(unit > 0, err / (K * unit), np.where(err > 0, np.inf, 0.0))


def _starts(k, f, D, window, lmax):
    """starts that cross every edge of file f: block boundaries and one either side, a negative one, one across the file's
    end, one inside the tail, one wholly past the tail"""
    n = int(k.index[f]["n_samples"]) // D
    edge = k.boundaries(f, D)[len(k.boundaries(f, D)) // 2]
    return [edge - 1, edge, edge + 1, 0, -37, n - window // 2 - 1, n + 5, n + lmax + 3]


def test_the_block_is_the_librarys():
    from mrcaudiocodec_amd import _lib, store
    assert store.REVERB_BLOCK == _lib.MRC_STORE_REVERB_BLOCK == B and store.MAX_IR_TAPS == 1 << 17


# ------------------------------------------------------------------ 1: accuracy over every edge of length, window and start
@pytest.mark.parametrize("window", WINDOWS)
def test_convolved_terms_meet_the_bound(kitchen, window):
    k = kitchen
    rows = []
    for f in range(len(k.files)):
        starts = _starts(k, f, 1, window, LENGTHS[-1])
        rows += [[(f, starts[(i + f) % len(starts)], 1.0, i)] for i in range(len(LENGTHS))]
    got = _call(k, rows, window, channels=2, dtype=torch.float64).cpu().numpy()
    ref, unit, numpy_ratio = _reference(k, rows, window, channels=2)
    excess = _excess(got, ref, unit)
    print("window %d: largest error %.3g of the bound (K = %g); NumPy's FFT convolution %.3g of the scale" % (window, excess.max(), K, numpy_ratio))
    assert numpy_ratio <= NUMPY_RATIO, "K rests on a ratio of %g, NumPy shows %g here" % (NUMPY_RATIO, numpy_ratio)
    assert np.all(excess <= 1.0), (window, [(rows[i], float(excess[i])) for i in np.flatnonzero(excess > 1.0)[:4]])
    assert np.abs(got).max() > 1e-3
    # a window wholly past the tail is zeros
    past = [i for i, row in enumerate(rows) if row[0][1] >= int(k.index[row[0][0]]["n_samples"]) + len(k.bank[row[0][3]]) - 1]
    assert past and not got[past].any()
    # ... and one inside the tail, past the file's end, is not (the response rings on)
    tail = [i for i, row in enumerate(rows) if row[0][1] == int(k.index[row[0][0]]["n_samples"]) + 5 and len(k.bank[row[0][3]]) > B]
    assert tail and all(got[i].any() for i in tail)


def test_the_bound_refuses_a_float32_twiddle_and_a_dropped_partition(kitchen):
    k = kitchen
    window = B + 1
    rows = [[(0, 100, 1.0, LENGTHS.index(2 * B + 1))], [(0, 300, 0.5, LENGTHS.index(3 * B + 17))]]
    got = _call(k, rows, window, channels=2, dtype=torch.float64).cpu().numpy()
    ref, unit, _ = _reference(k, rows, window, channels=2)
    assert np.all(_excess(got, ref, unit) <= 1.0)
    # a float32 twiddle: relative errors of 2^-24 in the transforms' outputs
    rms = np.sqrt(np.mean(np.square(ref.astype(np.float64))))
    noise = np.random.default_rng(3).standard_normal(ref.shape) * rms * 2.0 ** -24
    assert np.all(_excess(got, ref + noise, unit) > 1.0)
    # a dropped partition: the response without its second block of B taps
    bank = [h.copy() for h in k.bank]
    for h in bank:
        h[B:2 * B] = 0.0
    dropped, _, _ = _reference(k, rows, window, bank=bank, channels=2)
    assert np.all(_excess(got, dropped, unit) > 1.0)


# ------------------------------------------------------------------ 2: rows of mixed terms under every other argument
def _mixed_rows(k, D, window, n_ratio):
    """rows of 0, 1, 2 and 5 terms, convolved and not, over the files, starts and responses in turn -> rows, speed indices"""
    rng = np.random.default_rng(11 + D)
    gains = (1.0, -1.0, 0.3, 1e-3, 3.7)
    rows, at = [], 0
    for count in (2, 0, 1, 5, 1, 2, 5, 2):
        row = []
        for _ in range(count):
            f = at % len(k.files)
            starts = _starts(k, f, D, window, LENGTHS[-1])
            ir = -1 if at % 3 == 1 else (at * 5) % len(LENGTHS)
            row.append((f, starts[at % len(starts)] * 2 // 3 if n_ratio > 1 else starts[at % len(starts)], gains[at % len(gains)], ir))
            at += 1
        rows.append(row)
    rows.append([(0, 7, 0.5, -1), (len(k.files) - 1, 9, -2.0, -1)])                # no term convolved
    rows.append([(0, -5, 1.0, -1)])
    rows.append([(0, 64, 40.0, 1), (0, 64, 40.0, -1)])                             # past full scale: the 16-bit code saturates
    n_terms = sum(len(r) for r in rows)
    return rows, rng.integers(0, n_ratio, n_terms)


@pytest.mark.parametrize("D,mix,ratio,bands", [(1, None, None, False), (2, "mid", (2, 3), False), (4, "left", "speeds", True),
                                               (1, "mid", "speeds", False), (2, None, None, True), (4, None, (2, 3), False)])
def test_rows_of_mixed_terms_compose_with_the_other_arguments(kitchen, D, mix, ratio, bands):
    from mrcaudiocodec_amd.store import critical_band_edges
    k = kitchen
    window = 257
    rows, pick = _mixed_rows(k, D, window, 3 if ratio == "speeds" else 1)
    n_terms = len(pick)
    kw = dict(rate_divisor=D, mix=mix)
    if mix is None:
        kw["channels"] = 2
    if ratio == "speeds":
        kw.update(SPEEDS, speed_index=pick)
    elif ratio is not None:
        kw["resample"] = ratio + (ZEROS, ROLLOFF)
    if bands:
        nb = critical_band_edges(k.h.cfg.sample_rate).size - 1
        kw["band_gains"] = np.random.default_rng(5).uniform(0.25, 1.5, (n_terms, nb))
    got = _call(k, rows, window, dtype=torch.float64, **kw)
    ref, unit, _ = _reference(k, rows, window, **kw)
    excess = _excess(got.cpu().numpy(), ref, unit)
    print("D %d mix %s ratio %s bands %s: largest error %.3g of the bound" % (D, mix, ratio, bands, excess.max()))
    assert np.all(excess <= 1.0), [(rows[i], float(excess[i])) for i in np.flatnonzero(excess > 1.0)[:4]]
    assert float(got.abs().max()) > 1.0 and not bool(got[1].any())                 # (row 1 has no terms: +0.0)
    assert not bool(torch.signbit(got[1]).any())
    # the other formats are conversions of the float64 rows of the same call
    i16, f32 = _call(k, rows, window, **kw), _call(k, rows, window, dtype=torch.float32, **kw)
    assert i16.dtype == torch.int16 and np.array_equal(i16.cpu().numpy(), odec.pcm16(got.cpu().numpy()))
    assert int(i16[-1].to(torch.int32).abs().max()) == 32767
    assert f32.dtype == torch.float32 and np.array_equal(f32.cpu().numpy(), got.cpu().numpy().astype(np.float32))
    # rows none of whose terms is convolved are the existing call's, bit for bit, in all three formats -- inside this call ...
    files, starts, gains, irs, offsets = _flat(rows)
    dry_rows = [r for r in range(len(rows)) if len(rows[r]) and all(t[3] < 0 for t in rows[r])]
    assert len(dry_rows) >= 2
    for dtype, mine in ((torch.float64, got), (torch.float32, f32), (torch.int16, i16)):
        want = k.store.decode_window_sum(files, starts, gains, window, item_offsets=offsets, dtype=dtype, **kw)
        assert all(_same(mine[r], want[r]) for r in dry_rows)
        # ... and in a call without any convolved term
        alone = k.store.decode_window_sum(files, starts, gains, window, item_offsets=offsets, dtype=dtype,
                                          ir_index=np.full(n_terms, -1), **kw)
        assert _same(alone, want)
    assert k.store.reverb_ms() == {"forward": 0.0, "fold": 0.0}


# ------------------------------------------------------------------ 3: structure
def test_delays_the_unit_response_and_zero(kitchen):
    from mrcaudiocodec_amd.store import PacStore
    k = kitchen
    window, d = B + 1, B + 3
    delay = np.zeros(d + 1)
    delay[d] = 1.0
    with PacStore(k.h, k.files) as store:
        store.set_impulse_responses([delay, [1.0], [0.0]])
        assert store.impulse_response_lengths.tolist() == [d + 1, 1, 1]
        seen = 0
        for f in range(len(k.files)):
            n = int(k.index[f]["n_samples"])
            for start in (0, 411, n - 100):
                rows = [[(f, start, 1.0, 0)], [(f, start, 1.0, 1)], [(f, start, 1.0, 2)], [(f, start, -0.75, 0)]]
                got = _call(k, rows, window, store=store, channels=2, dtype=torch.float64).cpu().numpy()
                plain = _existing(k, [f, f], [start - d, start], window, store=store, channels=2)
                unit = RV.error_scale([1.0], _existing(k, [f], [start - d], window + d, store=store, channels=2), N_FFT)
                seen += int(plain[0].any()) + int(plain[1].any())
                assert np.abs(got[0] - plain[0]).max() <= K * unit                             # the window, d samples late
                assert np.abs(got[1] - plain[1]).max() <= K * unit                             # the window itself
                assert not got[2].any()                                                        # zeros
                assert np.abs(got[3] - -0.75 * got[0]).max() <= 2 * K * 0.75 * unit            # linear in the gain
        assert seen >= 3 * len(k.files)


def _silent_right_file():
    """three long blocks of a stereo file whose right channel is digital silence (every band is then coded L / R and the right
    channel's lines are zero)"""
    L, rate = 1024, 48000
    cp = ocodec.default_params(sampleRate=rate, nChannels=2, targetBitsPerSample=2.86)
    cp.nMDCTLines = cp.nSamplesPerBlock = cp.a = cp.b = L
    cp.nSamplesShort = 128
    cp.sfBands = ocodec.bands_for_block(L, L, L, rate)
    cp.bitReservoir = 0
    n = 3 * L
    t = np.arange(n)
    x = 0.25 * np.sin(2 * np.pi * 1000.0 / rate * t) + 0.05 * np.random.default_rng(2).standard_normal(n)
    pcm = np.zeros((2, n + L), np.int16)
    pcm[0, L:] = np.clip(np.rint(x * 32767.5), -32767, 32767).astype(np.int16)
    import settings_kit as SK
    return opac.encode_stereo_stream(SK.to_float(pcm), [(i * L, L, L) for i in range(3)], cp, huffman=True)


def test_a_silent_right_channel_stays_silent_within_the_bound():
    from mrcaudiocodec_amd.store import PacStore
    k = _kitchen_of("default")
    window, h = 700, RV.room(B + 1, 9)
    with PacStore(k.h, [_silent_right_file()]) as store:
        store.set_impulse_responses([h])
        dry = _existing(k, [0], [300 - B], window + B, store=store, channels=2)[0]
        assert dry[0].any() and not dry[1].any()
        got = store.decode_window([0], [300], window, channels=2, dtype=torch.float64, ir_index=[0])[0].cpu().numpy()
        unit = RV.error_scale(h, dry, N_FFT)
        print("silent right channel: largest value %.3g of the bound" % (np.abs(got[1]).max() / (K * unit)))
        assert np.abs(got[1]).max() <= K * unit                                                # nothing leaks between the packed channels
        assert np.abs(got[0] - RV.wet_reference(h, dry[0]).astype(np.float64)).max() <= K * unit and np.abs(got[0]).max() > 0.1


# ------------------------------------------------------------------ 4: equality to the bit
def test_a_convolved_term_depends_on_itself_alone(kitchen):
    from mrcaudiocodec_amd.store import PacStore
    k = kitchen
    window = B + 1
    rows, _ = _mixed_rows(k, 1, window, 1)
    kw = dict(channels=2, dtype=torch.float64)
    base = _call(k, rows, window, **kw)
    assert k.store.stats()["slabs"] == 1 and k.store.reverb_ms()["fold"] > 0.0
    assert _same(_call(k, rows, window, **kw), base)                                           # repeated calls
    order = np.random.default_rng(4).permutation(len(rows))
    assert _same(_call(k, [rows[i] for i in order], window, **kw), base[torch.as_tensor(order)])
    # company: every row alone, where Lpre is the row's own longest response and not the call's
    for i, row in enumerate(rows):
        assert _same(_call(k, [row], window, **kw)[0], base[i]), i
    # the slab size: one row per slab, a few rows per slab, one slab
    converted = {dtype: _call(k, rows, window, channels=2, dtype=dtype) for dtype in (torch.float32, torch.int16)}
    try:
        for slab, least in ((1, len(rows) - 1), (12 * (window + LENGTHS[-1]), 2), (0, 1)):
            k.h.set_option(SLAB_OPTION, slab)
            assert _same(_call(k, rows, window, **kw), base) and k.store.stats()["slabs"] >= least
            for dtype, want in converted.items():                                              # the conversions, slab by slab
                assert _same(_call(k, rows, window, channels=2, dtype=dtype), want)
    finally:
        k.h.set_option(SLAB_OPTION, SLAB_DEFAULT)
    # the bank: the same responses at other indices, among others
    with PacStore(k.h, k.files) as store:
        order = [5, 0, 7, 2, 4, 1, 6, 3]
        store.set_impulse_responses([RV.room(77, 1)] + [k.bank[i] for i in order] + [RV.room(2 * B + 5, 2)])
        where = {ir: 1 + order.index(ir) for ir in range(len(LENGTHS))}
        assert _same(_call(k, rows, window, store=store, bank_map=where, **kw), base)
    # decode_window(ir_index=) is the one-term row at gain 1.0
    files, starts, gains, irs, _ = _flat(rows)
    for dtype in (torch.float64, torch.float32, torch.int16):
        one = k.store.decode_window(files, starts, window, channels=2, dtype=dtype, ir_index=irs)
        want = k.store.decode_window_sum(files, starts, np.ones(len(files)), window, item_offsets=np.arange(len(files) + 1), channels=2,
                                         dtype=dtype, ir_index=irs)
        assert _same(one, want)
    dry = np.flatnonzero(irs < 0)
    f64 = k.store.decode_window(files, starts, window, channels=2, dtype=torch.float64, ir_index=irs)
    assert _same(f64[torch.as_tensor(dry)], k.store.decode_window(files[dry], starts[dry], window, channels=2, dtype=torch.float64))


# ------------------------------------------------------------------ 5: work and state
def test_work_follows_the_lengthened_spans_and_the_bank_is_state(kitchen):
    from mrcaudiocodec_amd import MrcError
    from mrcaudiocodec_amd.store import PacStore
    k = kitchen
    window = 300
    rows = [[(0, 2000, 1.0, 1), (0, 100, 0.5, -1)], [(len(k.files) - 1, 50, 1.0, LENGTHS.index(B + 1))]]
    files, starts, gains, irs, offsets = _flat(rows)
    with PacStore(k.h, k.files) as store:
        store.set_impulse_responses(k.bank)
        assert store.impulse_response_lengths.tolist() == LENGTHS
        _call(k, rows, window, store=store, channels=2, dtype=torch.float64)
        st, ms = store.stats(), store.reverb_ms()
        _existing(k, files, starts - B, window + B, store=store, channels=2)                  # the spans the call reads: Lpre = B
        want = store.stats()
        assert st["chunks_parsed"] == want["chunks_parsed"] > 0 and st["decode_launches"] == want["decode_launches"]
        assert ms["forward"] > 0.0 and ms["fold"] > 0.0 and st["ms"]["window_out"] >= ms["forward"] + ms["fold"]
        _existing(k, files, starts, window, store=store, channels=2)
        assert store.stats()["chunks_parsed"] < st["chunks_parsed"]
        # a new bank replaces the old one
        first = _call(k, rows, window, store=store, channels=2, dtype=torch.float64)
        store.set_impulse_responses([k.bank[1] * 2.0, k.bank[1]])
        assert store.impulse_response_lengths.tolist() == [2, 2]
        with pytest.raises(ValueError, match=r"ir_index must be -1 or lie in 0\.\.1"):
            _call(k, rows, window, store=store, channels=2, dtype=torch.float64)
        two = store.decode_window([0, 0], [2000, 2000], window, channels=2, dtype=torch.float64, ir_index=[0, 1])
        assert _same(two[1], k.store.decode_window([0], [2000], window, channels=2, dtype=torch.float64, ir_index=[1])[0])
        assert not _same(two[0], two[1]) and first.shape == (2, 2, window)
        # a refused bank leaves the old one
        rc = _set_irs_raw(store, [0, 1], [float("nan")])
        assert rc == -1 and "taps[0]" in _last_error(k)
        assert _same(store.decode_window([0, 0], [2000, 2000], window, channels=2, dtype=torch.float64, ir_index=[0, 1]), two)
        # no bank: an index is refused, by Python and by the library
        store.set_impulse_responses(None)
        assert store.impulse_response_lengths.size == 0
        with pytest.raises(ValueError, match="the store has none"):
            store.decode_window([0], [0], window, ir_index=[0])
        rc, out = _raw(k, store=store)
        text = _last_error(k)
        assert rc == -1 and bool((out == 77).all()) and "has no impulse responses" in text and "ir_of of term 0 = 0" in text
        assert _same(store.decode_window([0], [9], window, channels=2, ir_index=[-1]), store.decode_window([0], [9], window, channels=2))
        store.set_impulse_responses([[1.0, 0.5]])                                              # ... and closes with a bank set
    with pytest.raises(MrcError):
        store.set_impulse_responses([[1.0]])


# ------------------------------------------------------------------ 6: the library's refusals
def _last_error(k):
    from mrcaudiocodec_amd import _lib
    return _lib.lib.mrc_last_error(k.h._h).decode()


def _set_irs_raw(store, offsets, taps, n=None):
    from mrcaudiocodec_amd import _lib
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)
    offsets, taps = arr(offsets, np.int64), arr(taps, np.float64)
    ptr = lambda a: None if a is None else a.ctypes.data
    return _lib.lib.mrc_pac_store_set_irs(store._s, (offsets.size - 1) if n is None else n, ptr(offsets), ptr(taps))


def _raw(k, store=None, D=1, mix=3, ups=(1, 2), downs=(1, 3), n_ratios=None, zeros=16, rolloff=0.9, n_bands=0, edges=None, band_gain=None,
         offsets=(0, 2), files=(0, 0), starts=(0, 9), gains=(1.0, 0.5), ratio_of=(0, 1), ir_of=(0, -1), window=16, channels=2, fmt=None,
         out="tensor", n_items=None):
    """the entry point itself -> (status, the pre-filled tensor)"""
    from mrcaudiocodec_amd import _lib
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)
    ups, downs, ratio_of, ir_of = arr(ups, np.int32), arr(downs, np.int32), arr(ratio_of, np.int32), arr(ir_of, np.int32)
    offsets, files, starts = arr(offsets, np.int64), arr(files, np.int64), arr(starts, np.int64)
    gains, edges, band_gain = arr(gains, np.float64), arr(edges, np.float64), arr(band_gain, np.float64)
    ptr = lambda a: None if a is None else a.ctypes.data
    n = (offsets.size - 1 if offsets is not None else 1) if n_items is None else n_items
    t = torch.full((max(n, 1), channels if channels in (1, 2) else 2, window if 0 < window <= 4096 else 16), 77, dtype=torch.float64,
                   device=torch.device("cuda", 0))
    rc = _lib.lib.mrc_pac_store_decode_window_reverb(
        (store or k.store)._s, D, mix, (ups.size if ups is not None else 1) if n_ratios is None else n_ratios, ptr(ups), ptr(downs), zeros,
        rolloff, n_bands, ptr(edges), ptr(band_gain), n, ptr(offsets), ptr(files), ptr(starts), ptr(gains), ptr(ratio_of), ptr(ir_of),
        window, channels, _lib.MRC_WINDOW_F64 if fmt is None else fmt, t.data_ptr() if out == "tensor" else None, None)
    return rc, t


def test_library_refusals_come_before_any_device_work(kitchen):
    from mrcaudiocodec_amd import _lib
    k = kitchen
    fn = "mrc_pac_store_decode_window_reverb: "
    cases = [
        # the speeds call's, under this call's name
        (dict(D=3), ("rate_divisor 3",)), (dict(mix=7), ("mix 7",)), (dict(channels=1), ("term 0: file 0 is stereo",)),
        (dict(files=[0, len(k.files)]), ("file[1]", "outside the store")), (dict(window=-1), ("window",)),
        (dict(window=(1 << 40) + 1), ("window",)), (dict(fmt=9), ("format 9",)), (dict(out=None), ("out is NULL",)),
        (dict(offsets=[1, 2]), ("term_offset[0] = 1",)), (dict(gains=[1.0, float("nan")]), ("gain of term 1 is not finite",)),
        (dict(n_ratios=9), ("n_ratios 9", "1..8")), (dict(ratio_of=None), ("ratio_up, ratio_down or ratio_of is NULL",)),
        (dict(ratio_of=[0, 2]), ("ratio_of of term 1 = 2",)), (dict(edges=[0.0, 1000.0]), ("n_bands is 0",)),
        (dict(ups=[1, 1], downs=[1, 9]), ("ratio 1: down 9",)),
        # ... and its own
        (dict(ir_of=None), ("ir_of is NULL",)),
        (dict(ir_of=[0, len(LENGTHS)]), ("ir_of of term 1 = %d" % len(LENGTHS), "bank of %d impulse responses" % len(LENGTHS))),
        (dict(ir_of=[-2, 0]), ("ir_of of term 0 = -2", "neither -1 nor inside the bank")),
        (dict(window=(1 << 40) - 5, ir_of=[LENGTHS.index(B), -1]), ("window + the longest impulse response named - 1", "exceeds 2^40")),
    ]
    for change, words in cases:
        rc, out = _raw(k, **change)
        text = _last_error(k)
        assert rc == _lib.MRC_ERR_INVALID and bool((out == 77).all()), (change, rc, text)
        assert text.startswith(fn) and all(w in text for w in words), (change, text)
    for change in (dict(offsets=[0], files=None, starts=None, gains=None, ratio_of=None, ir_of=None), dict(window=0)):
        rc, out = _raw(k, **change)
        assert rc == 0 and bool((out == 77).all()), change
    rc, out = _raw(k)
    assert rc == 0 and bool((out != 77).all())
    rc, out = _raw(k, offsets=[0, 0, 2], ir_of=[3, -1])                                        # a row without terms: +0.0
    assert rc == 0 and not bool(out[0].any()) and bool(out[1].any())
    # the bank's own refusals: each names its argument and leaves the bank as it was
    fn = "mrc_pac_store_set_irs: "
    for args, words in ((dict(offsets=[0, 1], taps=[1.0], n=-1), ("n_irs < 0",)), (dict(offsets=None, taps=[1.0], n=1), ("ir_offset or taps is NULL",)),
                        (dict(offsets=[0, 1], taps=None), ("ir_offset or taps is NULL",)), (dict(offsets=[1, 2], taps=[1.0, 2.0]), ("ir_offset[0] = 1",)),
                        (dict(offsets=[0, 2, 2], taps=[1.0, 2.0]), ("impulse response 1 has 0 taps", "1..131072")),
                        (dict(offsets=[0, (1 << 17) + 1], taps=np.zeros((1 << 17) + 1)), ("impulse response 0 has 131073 taps",)),
                        (dict(offsets=[0, 1, 3], taps=[1.0, 2.0, float("inf")]), ("taps[2] (impulse response 1) is not finite",))):
        rc = _set_irs_raw(k.store, **args)
        text = _last_error(k)
        assert rc == _lib.MRC_ERR_INVALID and text.startswith(fn) and all(w in text for w in words), (args, text)
    assert k.store.impulse_response_lengths.tolist() == LENGTHS
    count, lengths = np.zeros(1, np.int64), np.zeros(len(LENGTHS), np.int64)
    assert _lib.lib.mrc_pac_store_ir_info(k.store._s, count.ctypes.data, lengths.ctypes.data) == 0
    assert int(count[0]) == len(LENGTHS) and lengths.tolist() == LENGTHS


# ------------------------------------------------------------------ 7: the command line
def test_cli_reverberates_through_the_store(tmp_path, capsys):
    from mrcaudiocodec_amd import cli
    from mrcaudiocodec_amd.store import PacStore
    k = _kitchen_of("default")
    a, dst, npy, wav = str(tmp_path / "a.pac"), str(tmp_path / "x.wav"), str(tmp_path / "ir.npy"), str(tmp_path / "ir.wav")
    with open(a, "wb") as fp:
        fp.write(k.files[0])
    h = RV.room(B + 7, 21)
    np.save(npy, h)
    n = int(k.index[0]["n_samples"])
    with PacStore(k.h, [k.files[0]]) as store:
        store.set_impulse_responses([h])
        want = store.decode_window([0], [0], n, dtype=torch.int16, ir_index=[0])[0].cpu().numpy()
        cli.main(["-d", a, dst, "--ir", npy])
        assert open(dst, "rb").read() == cli.wav_bytes(want, 48000) and want.shape == (2, n) and want.any()
        # a mono 16-bit WAV response, at 16 kHz mid and a speed
        codes = np.clip(np.rint(h[:300] * 16000), -32767, 32767).astype(np.int16)
        with open(wav, "wb") as fp:
            fp.write(cli.wav_bytes(codes[None], 16000))
        store.set_impulse_responses([cli.read_ir(wav, 16000)])
        m = int(store.n_samples_resampled(20, 33, 2)[0])
        want = store.decode_window([0], [0], m, dtype=torch.int16, rate_divisor=2, mix="mid", resample=(20, 33), ir_index=[0])[0].cpu().numpy()
        cli.main(["-d", a, dst, "--ir", wav, "--speed", "11/10", "--sample-rate", "16000", "--mix", "mid"])
        assert open(dst, "rb").read() == cli.wav_bytes(want, 16000) and want.shape == (1, m) and want.any()
    capsys.readouterr()
