"""
GPU tests of the store's STFT (mrc_pac_store_stft_window, PacStore.stft_window, cli --stft-energies).

The row under a transform is always the EXISTING call, decode_window_sum(..., dtype=float64) at window L = (n_frames - 1) hop +
n_fft -- the code this call is built around, not the code under test.

Accuracy.  The reference of a frame is a direct DFT in np.longdouble (tests/stft_reference.py) of the float64 products g * x of
that row.  The allowed error per bin of frame m is K * u_m, u_m = 2^-52 * log2(n_fft) * ||g x_m||_2, and K is 8 times the
largest error NumPy's own float64 real transform shows against the same reference on the very frames of
test_complex_bins_meet_the_bound, in the same unit: that ratio was measured as NUMPY_RATIO below (the test measures it again
and holds it to the record), which leaves room for another factorisation and for the pass that takes the real frame's two
halves apart.  The kernel transforms every frame by itself (one complex transform of n_fft / 2 points), so the sizes below
are read as: 16 = 2 * (4 * 2), 20 = 2 * (2 * 5), 30 = 2 * (3 * 5), 400 = 2 * (4 * 2 * 5 * 5), 480 = 2 * (4 * 4 * 3 * 5), 512 = 2 * 4^4,
1024 = 2 * (4^4 * 2), 2048 = 2 * 4^5 -- radix 5 after a power of two and after a 3, at two depths.  The kernel gives a transform 64
threads up to 512 points, 128 up to 1024 and 256 above: 1024 is there for the middle width.  A workgroup takes a run of F
frames and works them in rounds of 256 / (threads per transform), reusing the transform buffers while the assembled outputs
stay live: 13 frames (5 at n_fft 1024) make runs of several rounds and a tail run.  COMPLEX output takes twice the assembly
space, so against the long-double reference it runs three rounds (F = 12 + 1) at n_fft 16, 20 and 30, one round of four at 400
to 512 and single frames from 1024 on; the long runs of the larger sizes (POWER and BANK: F = 12 + 1 in three rounds at 400 /
160, 8 + 5 in two at 512, 4 + 1 in two rounds of two at 1024) are held TO THE BIT to that COMPLEX output of the same arguments
by test 2, and run in all three modes by the independence test.  At 2048 a run is one frame whatever the arguments.
Measured on an MI355X (each test prints its figures): NumPy 0.70, 0.69, 0.94, 1.21, 2.12, 1.65, 1.88, 1.65 units at the eight sizes, so
NUMPY_RATIO = 2.13 and K = 17.04; the kernel 0.70, 0.95, 0.94, 1.46, 1.81, 1.59, 2.04, 2.14 units, at most 0.126 of the bound; the
mixture through a room 1.09 units.
Everything else is equality to the bit: POWER and BANK given COMPLEX, the float32 conversions, independence of order,
company, slab size and the bank's order, repeated calls, center=True.
Files: those of tests/test_gpu_store_reduced.py (settings `default` and `B`), with the reverb test's bank.
"""
import numpy as np
import pytest

import chain_kit as kit  # noqa: F401
from chain_kit import handles_closed_after_module  # noqa: F401
import reverb_reference as RV
import stft_reference as SR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIDS = ("default", "B")
SLAB_OPTION, SLAB_DEFAULT = 7, 1 << 24
NUMPY_RATIO = 2.13                                   # NumPy's rfft: its largest error in units of u_m on the accuracy test's frames (2.12 measured, at n_fft 480)
K = 8 * NUMPY_RATIO
SIZES = (16, 20, 30, 400, 480, 512, 1024, 2048)
FRAMES = {1024: (1, 2, 3, 5), 2048: (1, 2, 3)}       # (the long-double reference stays in seconds); else 1, 2, 3, 7 and 13
LENGTHS = RV.bank_lengths(1024)
ZEROS, ROLLOFF = 16, 0.9475

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
    if a.dtype.is_complex:
        return a.dtype == b.dtype and _same(torch.view_as_real(a), torch.view_as_real(b))
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b) and torch.equal(torch.signbit(a), torch.signbit(b))


def _window(n_fft):
    """an asymmetric frame window without zeros: a reversed or shifted window cannot pass"""
    from mrcaudiocodec_amd.store import hann_window
    return hann_window(n_fft) * (1.0 + 0.5 * np.arange(n_fft) / n_fft) + 0.01


def _starts(k, f, D, window):
    """the reverb test's starts: around a block boundary, 0, a negative one, one across the file's end, two past it"""
    n = int(k.index[f]["n_samples"]) // D
    edge = k.boundaries(f, D)[len(k.boundaries(f, D)) // 2]
    return [edge - 1, edge, edge + 1, 0, -37, n - window // 2 - 1, n + 5, n + 3000]


def _existing(k, files, starts, L, **kw):
    """the EXISTING float64 rows: one-term rows at gain 1.0 unless gains= says otherwise -> numpy [n][channels][L]"""
    files, starts = np.asarray(files, np.int64), np.asarray(starts, np.int64)
    if "gains" not in kw:
        kw = dict(kw, gains=np.ones(files.size), item_offsets=np.arange(files.size + 1))
    gains = kw.pop("gains")
    return k.store.decode_window_sum(files, starts, gains, L, dtype=torch.float64, **kw).cpu().numpy()


def _check(got, x, g, n_fft, hop, n_frames, twiddle=None):
    """got complex [n][c][bins][frames] against the long-double DFT of the rows x [n][c][L] -> (the largest error in units of
    u_m, NumPy's largest ratio on the same frames)"""
    gx = (SR.frames_of(x, n_fft, hop, n_frames) * g).reshape(-1, n_fft)                     # [n c frames][n_fft], rounded once
    re, im = SR.dft(gx, twiddle)
    z = np.moveaxis(got, 2, 3).reshape(-1, n_fft // 2 + 1)
    return SR.ratio(z.real, z.imag, re, im, SR.unit(gx)), SR.numpy_ratio(gx, re, im)


def _variants(k):
    mono = [f for f in range(len(k.files)) if int(k.store.n_channels[f]) == 1]
    out = [(dict(channels=2), list(range(len(k.files)))), (dict(mix="mid"), list(range(len(k.files))))]
    return out + ([(dict(channels=1), mono)] if mono else [(dict(mix="left"), list(range(len(k.files))))])


RESULTS = {}


# ------------------------------------------------------------------ 1: accuracy of COMPLEX over sizes, hops, frame counts and starts
@pytest.mark.parametrize("n_fft", SIZES)
def test_complex_bins_meet_the_bound(kitchen, n_fft):
    k = kitchen
    g = _window(n_fft)
    per_call = max(1, min(8, 2048 // n_fft))
    worst, numpy_worst, turn, loud = 0.0, 0.0, 0, 0.0
    for hop in (1, n_fft // 4, n_fft, n_fft + 3):
        for n_frames in FRAMES.get(n_fft, (1, 2, 3, 7, 13)):
            L = (n_frames - 1) * hop + n_fft
            kw, pool = _variants(k)[turn % 3]
            files = [pool[(turn + i) % len(pool)] for i in range(per_call)]
            starts = [_starts(k, f, 1, L)[(turn + i) % 8] for i, f in enumerate(files)]
            turn += 1
            got = k.store.stft_window(files, starts, n_frames, hop, n_fft, frame_window=g, output="complex", dtype=torch.float64, **kw)
            assert got.dtype == torch.complex128 and got.shape[2:] == (n_fft // 2 + 1, n_frames) and got.shape[0] == per_call
            x = _existing(k, files, starts, L, **kw)
            err, ratio = _check(got.cpu().numpy(), x, g, n_fft, hop, n_frames)
            worst, numpy_worst, loud = max(worst, err), max(numpy_worst, ratio), max(loud, float(np.abs(x).max()))
            assert err <= K, (n_fft, hop, n_frames, kw, files, starts, err / K)
    RESULTS[(k.sid, n_fft)] = (worst / K, numpy_worst)
    print("n_fft %d (%s): largest error %.3g of the bound (K = %g); NumPy's rfft %.3g of the unit" % (n_fft, k.sid, worst / K, K, numpy_worst))
    assert numpy_worst <= NUMPY_RATIO, "K rests on a ratio of %g, NumPy shows %g here" % (NUMPY_RATIO, numpy_worst)
    assert loud > 1e-3


def test_the_bound_refuses_a_float32_twiddle_and_a_shifted_window(kitchen):
    k = kitchen
    n_fft, hop, n_frames = 400, 160, 3
    L, g = (n_frames - 1) * hop + n_fft, _window(400)
    files, starts = [0, 0], [100, 2500]
    got = k.store.stft_window(files, starts, n_frames, hop, n_fft, frame_window=g, output="complex", dtype=torch.float64, channels=2).cpu().numpy()
    x = _existing(k, files, starts, L, channels=2)
    assert np.abs(x).max() > 1e-3 and _check(got, x, g, n_fft, hop, n_frames)[0] <= K
    assert _check(got, x, g, n_fft, hop, n_frames, twiddle=np.float32)[0] > K               # twiddles rounded to float32
    assert _check(got, x, np.roll(g, 1), n_fft, hop, n_frames)[0] > K                       # the frame window one tap late
    assert _check(got, x[:, ::-1], g, n_fft, hop, n_frames)[0] > K                          # (and the channels swapped)


# ------------------------------------------------------------------ 2: POWER and BANK given COMPLEX, and the conversions
def _banks(n_fft, n_mel, rng):
    from mrcaudiocodec_amd.store import mel_bin_weights, mel_points
    bins = n_fft // 2 + 1
    extra = np.zeros((6, bins))
    extra[1, bins // 3] = 0.75                                       # a single entry (row 0: all zeros)
    extra[2] = rng.uniform(0.1, 1.0, bins) * np.where(np.arange(bins) % 3 == 0, -1.0, 1.0)   # dense over all bins, both signs
    extra[3, 2:6] = rng.uniform(0.1, 1.0, 4)                         # touches the next: [2, 6) and [6, 9)
    extra[4, 6:9] = rng.uniform(0.1, 1.0, 3)
    extra[5, 4:8] = rng.uniform(0.1, 1.0, 4)                         # overlaps both
    extra[5, 5] = 0.0                                                # (a zero INSIDE a support is used, as +0.0 * P)
    return np.vstack([mel_bin_weights(n_fft, 16000, mel_points(n_mel, 0.0, 8000.0)), extra])


def _fold(bank, power):
    """the left fold from +0.0 in ascending bin over each row's support, one rounding per product and per addition:
    power [n][c][bins][frames] -> [n][c][filters][frames]"""
    out = np.zeros(power.shape[:2] + (len(bank), power.shape[3]))
    for q, row in enumerate(bank):
        nz = np.flatnonzero(row)
        for kk in (range(nz[0], nz[-1] + 1) if nz.size else ()):
            out[:, :, q] = out[:, :, q] + row[kk] * power[:, :, kk]
    return out


@pytest.mark.parametrize("n_fft,n_mel,hop,n_frames", [(20, 5, 7, 7), (400, 80, 160, 13), (400, 80, 403, 2), (512, 40, 160, 13), (1024, 80, 480, 5), (2048, 80, 512, 3)])
def test_power_and_bank_are_bit_defined_given_the_bins(kitchen, n_fft, n_mel, hop, n_frames):
    k = kitchen
    files = [f % len(k.files) for f in range(3)]
    L = (n_frames - 1) * hop + n_fft
    starts = [_starts(k, f, 1, L)[i] for i, f in zip((0, 4, 5), files)]
    bank = _banks(n_fft, n_mel, np.random.default_rng(n_fft))
    call = lambda **kw: k.store.stft_window(files, starts, n_frames, hop, n_fft, channels=2, **kw)
    z = call(output="complex", dtype=torch.float64)
    p = call(output="power", dtype=torch.float64)
    e = call(output="bank", bank=bank, dtype=torch.float64)
    zn = z.cpu().numpy()
    want_p = zn.real * zn.real + zn.imag * zn.imag                   # each product rounded once, then added
    assert p.shape == (3, 2, n_fft // 2 + 1, n_frames) and np.array_equal(p.cpu().numpy(), want_p) and want_p.max() > 0
    want_e = _fold(bank, p.cpu().numpy())
    got_e = e.cpu().numpy()
    assert e.shape == (3, 2, len(bank), n_frames) and np.array_equal(got_e, want_e) and not np.signbit(got_e[:, :, n_mel]).any()
    assert not got_e[:, :, n_mel].any() and got_e[:, :, n_mel + 1].any() and got_e[:, :, :n_mel].max() > 0
    # float32 is one conversion of the float64 value
    assert _same(call(output="complex", dtype=torch.float32), z.to(torch.complex64))
    assert _same(call(output="complex", dtype=torch.complex64), z.to(torch.complex64))
    assert _same(call(output="power"), p.float()) and _same(call(output="bank", bank=bank), e.float())


# ------------------------------------------------------------------ 3: composition with every row argument
def test_a_mixture_through_a_room_meets_the_bound(kitchen):
    k = kitchen
    n_fft, hop, n_frames = 400, 160, 5
    L, g = (n_frames - 1) * hop + n_fft, _window(400)
    speech, noise = 0, len(k.files) - 1
    gains_db = np.linspace(3.0, -9.0, 25)
    rows = dict(gains=np.array([[1.0, 0.25], [0.5, 0.25]]), rate_divisor=2, mix="mid", resample=(2, 3, ZEROS, ROLLOFF),
                speed_factors=[(1, 1), (9, 10)], speed_index=[[1, 0], [1, 0]], ir_index=[[3, -1], [3, -1]],
                band_gains=np.stack([np.stack([10.0 ** (gains_db / 20.0), np.ones(25)])] * 2))
    files, starts = np.array([[speech, noise], [speech, noise]]), np.array([[700, 50], [-90, 1300]])
    got = k.store.stft_window(files, starts, n_frames, hop, n_fft, frame_window=g, output="complex", dtype=torch.float64, **rows)
    x = _existing(k, files, starts, L, **rows)                       # the existing reverb call's float64 rows
    assert got.shape == (2, 1, 201, n_frames) and x.shape == (2, 1, L) and np.abs(x).max() > 1e-3
    err, _ = _check(got.cpu().numpy(), x, g, n_fft, hop, n_frames)
    print("mixture through a room: largest error %.3g of the bound" % (err / K))
    assert err <= K
    assert k.store.stft_ms() > 0.0 and k.store.reverb_ms()["fold"] > 0.0


# ------------------------------------------------------------------ 4: independence, to the bit
@pytest.mark.parametrize("n_fft,hop,n_frames", [(400, 160, 13), (1024, 480, 5)])
def test_results_do_not_depend_on_order_company_slabs_or_the_banks_order(kitchen, n_fft, hop, n_frames):
    from mrcaudiocodec_amd.store import mel_bin_weights, mel_points
    k = kitchen
    # (POWER and BANK: runs of 12 frames in three rounds and a tail run of one; of 4 in two rounds of two and a tail at 1024)
    L = (n_frames - 1) * hop + n_fft
    files = np.array([f % len(k.files) for f in range(6)])
    starts = np.array([_starts(k, f, 1, L)[i] for i, f in enumerate(files)])
    bank = mel_bin_weights(n_fft, 16000, mel_points(12, 0.0, 8000.0))
    kw = dict(mix="mid", dtype=torch.float64)
    for mode in (dict(output="complex"), dict(output="power"), dict(output="bank", bank=bank)):
        base = k.store.stft_window(files, starts, n_frames, hop, n_fft, **mode, **kw)
        assert k.store.stats()["slabs"] == 1
        assert _same(k.store.stft_window(files, starts, n_frames, hop, n_fft, **mode, **kw), base)                  # a repeat
        perm = np.random.default_rng(5).permutation(len(files))
        assert _same(k.store.stft_window(files[perm], starts[perm], n_frames, hop, n_fft, **mode, **kw), base[perm])   # rows permuted
        for i in (0, 3):                                                                                            # a row alone
            assert _same(k.store.stft_window(files[i:i + 1], starts[i:i + 1], n_frames, hop, n_fft, **mode, **kw), base[i:i + 1])
        try:
            for slab, least in ((L, len(files)), (2 * L, len(files) // 2), (1, len(files))):                       # cut after every row, every second
                k.h.set_option(SLAB_OPTION, slab)
                assert _same(k.store.stft_window(files, starts, n_frames, hop, n_fft, **mode, **kw), base)
                assert k.store.stats()["slabs"] >= least
        finally:
            k.h.set_option(SLAB_OPTION, SLAB_DEFAULT)
    base = k.store.stft_window(files, starts, n_frames, hop, n_fft, output="bank", bank=bank, **kw)
    perm = np.random.default_rng(6).permutation(len(bank))
    assert _same(k.store.stft_window(files, starts, n_frames, hop, n_fft, output="bank", bank=bank[perm], **kw), base[:, :, perm])
    assert _same(k.store.stft_window(files, starts, n_frames, hop, n_fft, output="bank", bank=bank[3:5], **kw), base[:, :, 3:5])
    # center=True is starts moved by -n_fft // 2 and nothing else; the default window is the periodic Hann
    from mrcaudiocodec_amd.store import hann_window
    centred = k.store.stft_window(files, starts, n_frames, hop, n_fft, center=True, **kw)
    assert _same(centred, k.store.stft_window(files, starts - n_fft // 2, n_frames, hop, n_fft, frame_window=hann_window(n_fft), **kw))
    assert not _same(centred, k.store.stft_window(files, starts, n_frames, hop, n_fft, **kw))
    # rows of terms: a two-term row in company equals the row alone; a row without terms is +0.0
    offsets = np.array([0, 2, 2, 3])
    f3, s3, g3 = np.array([0, 0, 0]), np.array([100, 900, 100]), np.array([1.0, 0.5, 1.0])
    rows = k.store.stft_window(f3, s3, n_frames, hop, n_fft, gains=g3, item_offsets=offsets, **kw)
    assert rows.shape[0] == 3 and not rows[1].any() and not torch.signbit(rows[1]).any()
    assert _same(rows[2:], k.store.stft_window([0], [100], n_frames, hop, n_fft, **kw))
    assert _same(rows[:1], k.store.stft_window(f3[:2], s3[:2], n_frames, hop, n_fft, gains=g3[:2], item_offsets=[0, 2], **kw))


# ------------------------------------------------------------------ 5: the library's refusals
def _last_error(k):
    from mrcaudiocodec_amd import _lib
    return _lib.lib.mrc_last_error(k.h._h).decode()


def _raw(k, D=1, mix=3, ups=(1,), downs=(1,), n_ratios=None, n_bands=0, edges=None, band_gain=None, offsets=(0, 1, 2), files=(0, 0),
         starts=(0, 9), gains=(1.0, 0.5), ratio_of=(0, 0), ir_of=(-1, -1), n_fft=16, window="ones", n_frames=3, hop=4, mode=1, n_filters=0,
         bank=None, channels=2, fmt=None, out="tensor", n_items=None):
    """the entry point itself -> (status, the pre-filled tensor)"""
    from mrcaudiocodec_amd import _lib
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)
    ups, downs, ratio_of, ir_of = arr(ups, np.int32), arr(downs, np.int32), arr(ratio_of, np.int32), arr(ir_of, np.int32)
    offsets, files, starts = arr(offsets, np.int64), arr(files, np.int64), arr(starts, np.int64)
    gains, edges, band_gain, bank = arr(gains, np.float64), arr(edges, np.float64), arr(band_gain, np.float64), arr(bank, np.float64)
    window = arr(np.ones(max(n_fft, 1)) if isinstance(window, str) else window, np.float64)
    ptr = lambda a: None if a is None else a.ctypes.data
    n = (offsets.size - 1 if offsets is not None else 1) if n_items is None else n_items
    t = torch.full((16384,), 77, dtype=torch.float64, device=torch.device("cuda", 0))   # (2 x 2 x 1025 x 3 values at n_fft 2048)
    rc = _lib.lib.mrc_pac_store_stft_window(
        k.store._s, D, mix, (ups.size if ups is not None else 1) if n_ratios is None else n_ratios, ptr(ups), ptr(downs), ZEROS, ROLLOFF,
        n_bands, ptr(edges), ptr(band_gain), n, ptr(offsets), ptr(files), ptr(starts), ptr(gains), ptr(ratio_of), ptr(ir_of), n_fft,
        ptr(window), n_frames, hop, mode, n_filters, ptr(bank), channels, _lib.MRC_WINDOW_F64 if fmt is None else fmt,
        t.data_ptr() if out == "tensor" else None, None)
    return rc, t


def test_library_refusals_come_before_any_device_work(kitchen):
    from mrcaudiocodec_amd import _lib
    k = kitchen
    fn = "mrc_pac_store_stft_window: "
    nan_window = np.ones(16)
    nan_window[5] = np.nan
    inf_bank = np.ones((2, 9))
    inf_bank[1, 4] = np.inf
    cases = [
        # the reverb call's, under this call's name
        (dict(D=3), ("rate_divisor 3",)), (dict(mix=7), ("mix 7",)), (dict(channels=1), ("file 0 is stereo",)),
        (dict(files=[0, len(k.files)]), ("file[1]", "outside the store")), (dict(out=None), ("out is NULL",)),
        (dict(offsets=[1, 2, 2]), ("term_offset[0] = 1",)), (dict(gains=[1.0, float("nan")]), ("gain of term 1 is not finite",)),
        (dict(n_ratios=9), ("n_ratios 9", "1..8")), (dict(ratio_of=None), ("ratio_up, ratio_down or ratio_of is NULL",)),
        (dict(ratio_of=[0, 2]), ("ratio_of of term 1 = 2",)), (dict(edges=[0.0, 1000.0]), ("n_bands is 0",)),
        (dict(ir_of=None), ("ir_of is NULL",)), (dict(ir_of=[-2, 0]), ("ir_of of term 0 = -2",)),
        (dict(ir_of=[0, len(LENGTHS)]), ("ir_of of term 1 = %d" % len(LENGTHS),)),
        # ... and its own
        (dict(n_fft=14), ("n_fft 14",)), (dict(n_fft=22), ("n_fft 22",)), (dict(n_fft=401), ("n_fft 401",)), (dict(n_fft=2050), ("n_fft 2050",)),
        (dict(n_fft=4096), ("n_fft 4096",)), (dict(n_fft=0), ("n_fft 0",)), (dict(window=None), ("frame_window is NULL",)),
        (dict(window=nan_window), ("frame_window[5] is not finite",)), (dict(n_frames=-1), ("n_frames < 0",)), (dict(hop=0), ("hop < 1",)),
        (dict(n_frames=(1 << 40) - 14, hop=1), ("exceeds 2^40",)), (dict(n_frames=2, hop=1 << 40), ("exceeds 2^40",)),
        (dict(n_frames=(1 << 40) - 20, hop=1, ir_of=[LENGTHS.index(1024), -1]), ("L + the longest impulse response named - 1", "exceeds 2^40")),
        (dict(mode=3), ("mode 3",)), (dict(mode=-1), ("mode -1",)), (dict(fmt=_lib.MRC_WINDOW_PCM16), ("format 0",)), (dict(fmt=9), ("format 9",)),
        (dict(mode=2, n_filters=0, bank=np.ones((1, 9))), ("n_filters 0 outside 1..256",)),
        (dict(mode=2, n_filters=257, bank=np.ones((257, 9))), ("n_filters 257 outside 1..256",)),
        (dict(mode=2, n_filters=2), ("bank is NULL",)), (dict(mode=2, n_filters=2, bank=inf_bank), ("bank[1][4] is not finite",)),
        (dict(mode=1, n_filters=2), ("n_filters must be 0 and bank NULL",)), (dict(mode=0, bank=np.ones((1, 9))), ("n_filters must be 0 and bank NULL",)),
    ]
    for change, words in cases:
        rc, out = _raw(k, **change)
        text = _last_error(k)
        assert rc == _lib.MRC_ERR_INVALID and bool((out == 77).all()), (change, rc, text)
        assert text.startswith(fn) and all(w in text for w in words), (change, text)
    for change in (dict(offsets=[0], files=None, starts=None, gains=None, ratio_of=None, ir_of=None), dict(n_frames=0)):
        rc, out = _raw(k, **change)
        assert rc == 0 and bool((out == 77).all()), change
    for n_fft in (16, 18, 20, 30, 400, 2048):                        # the rule's other side; power of 2 rows x 2 channels x 3 frames
        rc, out = _raw(k, n_fft=n_fft, hop=1)
        used = 2 * 2 * (n_fft // 2 + 1) * 3
        assert rc == 0 and bool((out[:used] != 77).all()) and bool((out[used:] == 77).all()), (n_fft, _last_error(k))
    ms = np.zeros(1)
    assert _lib.lib.mrc_pac_store_stft_ms(k.store._s, ms.ctypes.data) == 0 and ms[0] > 0.0


# ------------------------------------------------------------------ 6: the command line
def test_cli_writes_the_python_calls_numbers(tmp_path, capsys):
    from mrcaudiocodec_amd import cli
    from mrcaudiocodec_amd.store import PacStore, hann_window, mel_bin_weights, mel_points, padded_window
    k = _kitchen_of("default")
    a, dst = str(tmp_path / "a.pac"), str(tmp_path / "e.npy")
    with open(a, "wb") as fp:
        fp.write(k.files[0])
    n = int(k.index[0]["n_samples"])
    with PacStore(k.h, [k.files[0]]) as store:
        # power at full rate, both channels, the whole file rounded down to whole frames
        frames = (n - 1024) // 480 + 1
        want = store.stft_window([0], [0], frames, 480, 1024, channels=2)[0].cpu().numpy()
        cli.main(["--stft-energies", a, dst, "--n-fft", "1024", "--hop", "480"])
        got = np.load(dst)
        assert got.dtype == np.float32 and got.shape == (2, 513, frames) and np.array_equal(got, want) and want.max() > 0
        # 80 mel filters of a 400-point Hann padded to 512 at 16 kHz mid, an excerpt
        m = 4000
        frames = (m - 512) // 160 + 1
        bank = mel_bin_weights(512, 16000, mel_points(80, 20.0, 7600.0, "slaney"), "slaney")
        want = store.stft_window([0], [300], frames, 160, 512, frame_window=padded_window(hann_window(400), 512), bank=bank, output="bank",
                                 rate_divisor=2, mix="mid", resample=(2, 3))[0].cpu().numpy()
        cli.main(["--stft-energies", a, dst, "--n-fft", "512", "--hop", "160", "--win-length", "400", "--mel", "80", "--f-min", "20", "--f-max", "7600",
                  "--mel-scale", "slaney", "--filter-norm", "slaney", "--sample-rate", "16000", "--mix", "mid", "--start", "300", "--samples", str(m)])
        got = np.load(dst)
        assert got.shape == (1, 80, frames) and np.array_equal(got, want) and want.max() > 0
        # complex bins
        want = store.stft_window([0], [0], 3, 100, 400, output="complex", channels=2)[0].cpu().numpy()
        cli.main(["--stft-energies", a, dst, "--n-fft", "400", "--hop", "100", "--samples", "600", "--complex"])
        got = np.load(dst)
        assert got.dtype == np.complex64 and np.array_equal(got, want)
    for argv, text in ((["--stft-energies", a, dst, "--hop", "160"], "--stft-energies needs --n-fft"),
                       (["--stft-energies", a, dst, "--n-fft", "400"], "--stft-energies needs --hop"),
                       (["--stft-energies", a, dst, "--n-fft", "22", "--hop", "4"], "n_fft must be an even int"),
                       (["--stft-energies", a, dst, "--n-fft", "400", "--hop", "160", "--complex", "--mel", "80"], "--complex"),
                       (["--stft-energies", a, dst, "--n-fft", "400", "--hop", "160", "--win-length", "401"], "--win-length"),
                       (["-d", a, dst, "--n-fft", "400"], "--n-fft belongs to --stft-energies")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2 and text in capsys.readouterr().err, argv
    capsys.readouterr()
