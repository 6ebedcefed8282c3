"""
GPU tests of the store's routed windows (mrc_pac_store_decode_window_routed, mrc_pac_store_stft_window_routed,
mrc_pac_store_route_info; PacStore.decode_window_routed / stft_window(route_gains=, route_irs=) / route_info, cli -d --array-ir).

Everything here is equality to the bit.  Channel c of a routed row is DEFINED as the one-channel row the reverb call gives over
the terms whose route to c is not absent, with that channel's gains and responses: the reference is
PacStore.decode_window_sum(ir_index=) -- the parent's call, whose own accuracy tests/test_gpu_store_reverb.py holds to its bound --
asked once per channel, and the comparison is torch.equal with equal sign bits in float64, float32 and int16.  No tolerance.
Files: those of tests/test_gpu_store_reduced.py, settings `default` (one stereo file: mid, left, right) and `B` (two stereo and
two mono files: mix None on the mono ones).  The bank: reverb_reference.bank_lengths(1024) plus four responses each of B - 1,
B + 1 and 2 B + 1 taps, so that arrays of equal lengths exist.
"""
import ctypes as C  # noqa: F401

import numpy as np
import pytest

import chain_kit as kit  # noqa: F401
from chain_kit import handles_closed_after_module  # noqa: F401
import reverb_reference as RV

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIDS = ("default", "B")
SLAB_OPTION, SLAB_DEFAULT = 7, 1 << 24
GROUP_OPTION = 8                                     # MRC_OPT_STORE_ROUTE_GROUP
B = 1024                                             # MRC_STORE_REVERB_BLOCK
LENGTHS = RV.bank_lengths(B) + [B - 1] * 4 + [B + 1] * 4 + [2 * B + 1] * 4
# the responses of one length: five each -- the one of bank_lengths and the four more
ARRAYS = {n: [i for i, v in enumerate(LENGTHS) if v == n] for n in (B - 1, B + 1, 2 * B + 1)}
NONE = -2                                            # MRC_ROUTE_NONE
CHANNELS = (1, 2, 3, 5, 16)
WINDOWS = (1, 257, B, B + 1, 2 * B + 1)
ZEROS, ROLLOFF = 16, 0.9475
SPEEDS = dict(resample=(2, 3, ZEROS, ROLLOFF), speed_factors=[(1, 1), (9, 10), (11, 10)])
# (D, mix, ratio, bands) as the reverb test composes them; the first on the mono files where the setting has them (B), else on
# the right channel of the stereo file
COMBOS = [(1, None, None, False), (2, "mid", (2, 3), False), (4, "left", "speeds", True)]
FORMATS = (torch.float64, torch.float32, torch.int16)

_KITCHENS = {}


def _kitchen_of(sid):
    from test_gpu_store_reduced import _Kitchen
    if sid not in _KITCHENS:
        k = _Kitchen(sid)
        k.bank = [RV.room(n, 100 + i) for i, n in enumerate(LENGTHS)]
        k.store.set_impulse_responses(k.bank)
        k.mono = [f for f in range(len(k.files)) if int(k.store.n_channels[f]) == 1]
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


def _starts(k, f, D, window, lmax):
    """the reverb test's pattern: block edges and one either side, a negative start, one across the file's end, one inside the
    tail, one wholly past the tail"""
    n = int(k.index[f]["n_samples"]) // D
    edge = k.boundaries(f, D)[len(k.boundaries(f, D)) // 2]
    return [edge - 1, edge, edge + 1, 0, -37, n - window // 2 - 1, n + 5, n + lmax + 3]


def _routes_of(kind, at, n_ch, live, rng):
    """the routes of one term to n_ch channels, of which the channels in `live` may be reached -> (gains, irs)"""
    gains = np.array([(1.0, -1.0, 0.3, 1e-3, 3.7)[(at + c) % 5] for c in range(n_ch)])
    irs = np.full(n_ch, NONE, np.int64)
    for j, c in enumerate(live):
        if kind == "array":                                  # every route wet, one length
            irs[c] = ARRAYS[(B + 1, 2 * B + 1, B - 1)[at % 3]][j % 5]
        elif kind == "two":                                  # wet routes of two different lengths
            irs[c] = ARRAYS[B + 1][(j // 2) % 5] if j % 2 == 0 else LENGTHS.index((3 * B + 17, 2)[(at // 4) % 2])
        elif kind == "drywet":                               # a dry and a wet route
            irs[c] = -1 if j % 2 == 0 else (at * 5 + j) % len(LENGTHS)
        else:                                                # drawn: absent, dry or any response
            irs[c] = (NONE, -1, int(rng.integers(0, len(LENGTHS))))[int(rng.integers(0, 3))]
    return gains, irs


def _rows(k, n_ch, window, D, files, scaled, seed=0):
    """rows of 0 to 4 terms -> files, starts, offsets, route gains [terms][n_ch], route irs [terms][n_ch].  From three channels
    on the last channel is absent for every term; below that every channel is live."""
    rng = np.random.default_rng(17 + seed + n_ch)
    live = list(range(n_ch - 1)) if n_ch >= 3 else list(range(n_ch))
    kinds = ("array", "two", "drywet", "drawn")
    fs, ss, gs, irs, offsets, at = [], [], [], [], [0], 0
    for count in (2, 0, 1, 4, 3):
        for _ in range(count):
            f = files[at % len(files)]
            starts = _starts(k, f, D, window, max(LENGTHS))
            s = starts[at % len(starts)]
            g, ir = _routes_of(kinds[at % 4], at, n_ch, live, rng)
            fs.append(f)
            ss.append(s * 2 // 3 if scaled else s)
            gs.append(g)
            irs.append(ir)
            at += 1
        offsets.append(len(fs))
    return (np.array(fs, np.int64), np.array(ss, np.int64), np.array(offsets, np.int64), np.array(gs, np.float64).reshape(-1, n_ch),
            np.array(irs, np.int32).reshape(-1, n_ch))


def _kw_of(k, combo, n_terms):
    """-> (the keyword arguments both calls share, the per-term ones as arrays to be cut per channel, the files to draw from)"""
    from mrcaudiocodec_amd.store import critical_band_edges
    D, mix, ratio, bands = combo
    files = list(range(len(k.files)))
    if mix is None:
        if k.mono:
            files = k.mono
        else:
            mix = "right"
    kw, per_term = dict(rate_divisor=D, mix=mix), {}
    if ratio == "speeds":
        kw.update(SPEEDS)
        per_term["speed_index"] = np.random.default_rng(3).integers(0, 3, n_terms)
    elif ratio is not None:
        kw["resample"] = ratio + (ZEROS, ROLLOFF)
    if bands:
        nb = critical_band_edges(k.h.cfg.sample_rate).size - 1
        per_term["band_gains"] = np.random.default_rng(5).uniform(0.25, 1.5, (n_terms, nb))
    return kw, per_term, files


def _channel_reference(k, c, files, starts, offsets, gains, irs, window, dtype, kw, per_term, store=None, bank_map=None):
    """channel c by the parent's call: the terms whose route to c is not absent -> [rows][window]"""
    keep = np.flatnonzero(irs[:, c] != NONE)
    if keep.size == 0:                                       # the contract's own words: +0.0
        return torch.zeros((len(offsets) - 1, window), dtype=dtype, device=torch.device("cuda", 0))
    row_of = np.searchsorted(offsets, keep, side="right") - 1
    offs = np.concatenate([[0], np.cumsum(np.bincount(row_of, minlength=len(offsets) - 1))]).astype(np.int64)
    ir = irs[keep, c]
    if bank_map is not None:
        ir = np.array([bank_map[i] if i >= 0 else -1 for i in ir], np.int32)
    cut = {name: v[keep] for name, v in per_term.items()}
    if kw.get("mix") is None:
        cut["channels"] = 1
    return (store or k.store).decode_window_sum(files[keep], starts[keep], gains[keep, c], window, item_offsets=offs, ir_index=ir,
                                                dtype=dtype, **kw, **cut)[:, 0]


def _routed(k, files, starts, offsets, gains, irs, window, dtype, kw, per_term, store=None, bank_map=None):
    if bank_map is not None:
        irs = np.where(irs >= 0, np.array([bank_map.get(i, 0) for i in range(len(LENGTHS))])[np.maximum(irs, 0)], irs).astype(np.int32)
    return (store or k.store).decode_window_routed(files, starts, gains, irs, window, item_offsets=offsets, dtype=dtype, **kw, **per_term)


# ------------------------------------------------------------------ 1: every channel is the parent's one-channel row
@pytest.mark.parametrize("n_ch", CHANNELS)
@pytest.mark.parametrize("combo", COMBOS, ids=["D1-each", "D2-mid-2/3", "D4-left-speeds-bands"])
def test_every_channel_is_the_reverb_calls_row(kitchen, combo, n_ch):
    k = kitchen
    for window in WINDOWS:
        kw, per_term, eligible = _kw_of(k, combo, 10)
        files, starts, offsets, gains, irs = _rows(k, n_ch, window, combo[0], eligible, combo[2] is not None)
        assert len(files) == 10
        if n_ch >= 3:                                        # what the rows must hold
            live = irs[:, :-1]
            lens = [{LENGTHS[v] for v in row if v >= 0} for row in live]
            assert any(np.all(row >= 0) and len(s) == 1 for row, s in zip(live, lens)) and any(len(s) == 2 for s in lens)
            assert any((row == -1).any() and (row >= 0).any() for row in live) and np.all(irs[:, -1] == NONE)
        for dtype in FORMATS:
            got = _routed(k, files, starts, offsets, gains, irs, window, dtype, kw, per_term)
            assert got.shape == (5, n_ch, window) and got.dtype == dtype
            for c in range(n_ch):
                want = _channel_reference(k, c, files, starts, offsets, gains, irs, window, dtype, kw, per_term)
                assert _same(got[:, c], want), (window, dtype, c)
            assert not bool(got[1].any())                    # (row 1 has no terms)
            if n_ch >= 3:                                    # a channel no term reaches: +0.0
                assert not bool(got[:, -1].any()) and (dtype == torch.int16 or not bool(torch.signbit(got[:, -1]).any()))
        if window > 1:
            assert float(got.to(torch.float64).abs().max()) > 0.0


# ------------------------------------------------------------------ 2: one channel is the reverb call
def test_one_channel_is_the_reverb_call_with_its_statistics(kitchen):
    k = kitchen
    window = B + 1
    kw, per_term, eligible = _kw_of(k, COMBOS[1], 10)
    files, starts, offsets, gains, irs = _rows(k, 1, window, 2, eligible, True)
    irs = np.where(irs == NONE, -1, irs).astype(np.int32)    # (an absent route has no counterpart in the reverb call)
    assert (irs >= 0).any() and (irs == -1).any()
    counters = lambda st: {name: st[name] for name in ("chunks_parsed", "decode_launches", "slabs", "plan_bytes_uploaded")}
    for dry in (False, True):                                # ... and without a wet route: both ARE the speeds call then
        ir = np.full_like(irs, -1) if dry else irs
        for dtype in FORMATS:
            got = _routed(k, files, starts, offsets, gains, ir, window, dtype, kw, per_term)
            mine, ms = counters(k.store.stats()), k.store.reverb_ms()
            want = k.store.decode_window_sum(files, starts, gains[:, 0], window, item_offsets=offsets, ir_index=ir[:, 0], dtype=dtype, **kw)
            assert _same(got, want) and mine == counters(k.store.stats()) and mine["chunks_parsed"] > 0
            assert (ms["fold"] == 0.0) == dry and (k.store.reverb_ms()["fold"] == 0.0) == dry


# ------------------------------------------------------------------ 3: independence
def test_a_channel_depends_on_its_own_routes_alone(kitchen):
    from mrcaudiocodec_amd.store import PacStore
    k = kitchen
    window, n_ch, dtype = B + 1, 5, torch.float64
    kw, per_term, eligible = _kw_of(k, COMBOS[1], 10)
    files, starts, offsets, gains, irs = _rows(k, n_ch, window, 2, eligible, True)
    irs[:, -1] = irs[:, 0]                                   # (all five channels live here)
    assert per_term == {}
    call = lambda rows=None, chans=None, **more: _routed(k, *_cut(files, starts, offsets, gains, irs, rows, chans), window, dtype, kw, {}, **more)
    base = call()
    assert k.store.stats()["slabs"] == 1 and float(base.abs().max()) > 0.0
    assert _same(call(), base)                                                                 # called twice
    order = [4, 2, 0, 3, 1]
    assert _same(call(rows=order), base[torch.as_tensor(order)])                               # the rows in another order
    assert _same(call(rows=order[::-1]), base[torch.as_tensor(order[::-1])])
    for r in range(5):
        assert _same(call(rows=[r])[0], base[r]), r                                            # one row alone
    try:                                                                                       # every row a slab of its own
        k.h.set_option(SLAB_OPTION, 1)
        assert _same(call(), base) and k.store.stats()["slabs"] >= 4
    finally:
        k.h.set_option(SLAB_OPTION, SLAB_DEFAULT)
    perm = [3, 0, 4, 2, 1]
    assert _same(call(chans=perm), base[:, torch.as_tensor(perm)])                             # the channels permuted
    assert _same(call(chans=[0, 3]), base[:, torch.as_tensor([0, 3])])                         # two of the five
    assert _same(call(chans=[3]), base[:, torch.as_tensor([3])])
    try:                                                                                       # how the kernel groups them
        for group in (1, 2):
            k.h.set_option(GROUP_OPTION, group)
            assert _same(call(), base) and _same(call(chans=perm), base[:, torch.as_tensor(perm)])
    finally:
        k.h.set_option(GROUP_OPTION, 0)                                                        # (the default: chosen per slab)
    with PacStore(k.h, k.files) as store:                                                      # the bank in another order
        order = list(np.random.default_rng(8).permutation(len(LENGTHS)))
        store.set_impulse_responses([RV.room(77, 1)] + [k.bank[i] for i in order] + [RV.room(2 * B + 5, 2)])
        where = {ir: 1 + order.index(ir) for ir in range(len(LENGTHS))}
        assert _same(call(store=store, bank_map=where), base)


def _cut(files, starts, offsets, gains, irs, rows, chans):
    """the rows `rows` (None: all) in that order and the channels `chans` (None: all) in that order"""
    if rows is not None:
        take = np.concatenate([np.arange(offsets[r], offsets[r + 1]) for r in rows]).astype(np.int64)
        offsets = np.concatenate([[0], np.cumsum([offsets[r + 1] - offsets[r] for r in rows])]).astype(np.int64)
        files, starts, gains, irs = files[take], starts[take], gains[take], irs[take]
    if chans is not None:
        gains, irs = np.ascontiguousarray(gains[:, chans]), np.ascontiguousarray(irs[:, chans])
    return files, starts, offsets, gains, irs


# ------------------------------------------------------------------ 4: the work is shared
def test_a_term_is_decoded_and_transformed_once(kitchen):
    from mrcaudiocodec_amd.store import array_routes
    k = kitchen
    window, n_ch = 2 * B + 1, 4
    M = -(-window // B)
    f = len(k.files) - 1
    files, starts = np.array([0, f, 0], np.int64), np.array([100, 50, 2000], np.int64)
    offsets = np.array([0, 2, 3], np.int64)
    kw = dict(mix="mid", dtype=torch.float64)
    # the bank room-major: room 1 of four microphones is responses 12..15 (B + 1 taps), room 0 is 8..11 -- as if rooms of four
    # started at response 8
    gains, irs = array_routes([1, 1, 1], n_ch)
    irs = irs + 8
    assert irs.tolist() == [ARRAYS[B + 1][1:]] * 3
    got = k.store.decode_window_routed(files, starts, gains, irs, window, item_offsets=offsets, **kw)
    st, info = k.store.stats(), k.store.route_info()
    one = k.store.decode_window_sum(files, starts, gains[:, 0], window, item_offsets=offsets, ir_index=irs[:, 0], **kw)
    want = k.store.stats()
    assert _same(got[:, 0], one[:, 0])
    assert st["chunks_parsed"] == want["chunks_parsed"] > 0 and st["decode_launches"] == want["decode_launches"]
    segments = lambda n: M + -(-n // B) - 1
    assert info["forward_segments"] == 3 * segments(B + 1)
    assert info["inverse_transforms"] == n_ch * 3 * M
    assert info["spectra_bytes"] == info["forward_segments"] * 2 * B * 16
    assert k.store.reverb_ms()["forward"] > 0.0 and k.store.reverb_ms()["fold"] > 0.0
    # two lengths on a term: a source per length
    irs2 = irs.copy()
    irs2[:, 1::2] = np.array(ARRAYS[2 * B + 1][:2])
    k.store.decode_window_routed(files, starts, gains, irs2, window, item_offsets=offsets, **kw)
    info = k.store.route_info()
    assert info["forward_segments"] == 3 * (segments(B + 1) + segments(2 * B + 1)) and info["inverse_transforms"] == n_ch * 3 * M
    # dry and absent routes transform nothing
    irs3 = irs.copy()
    irs3[:, 0], irs3[:, 1] = -1, NONE
    k.store.decode_window_routed(files, starts, gains, irs3, window, item_offsets=offsets, **kw)
    info = k.store.route_info()
    assert info["forward_segments"] == 3 * segments(B + 1) and info["inverse_transforms"] == 2 * 3 * M


# ------------------------------------------------------------------ 5: the STFT of routed rows
@pytest.mark.parametrize("n_fft,hop", [(16, 5), (400, 160)])
def test_stft_of_a_channel_is_stft_window_of_its_row(kitchen, n_fft, hop):
    k = kitchen
    n_ch, frames = 3, 3
    kw, per_term, eligible = _kw_of(k, COMBOS[1], 10)
    files, starts, offsets, gains, irs = _rows(k, n_ch, (frames - 1) * hop + n_fft, 2, eligible, True, seed=1)
    irs[:, -1] = np.where(np.arange(10) % 2 == 0, ARRAYS[B - 1][2], -1)                        # (three live channels)
    bank = np.abs(np.random.default_rng(2).standard_normal((4, n_fft // 2 + 1)))
    for output in ("complex", "power", "bank"):
        extra = dict(output=output, dtype=torch.float64, **kw)
        if output == "bank":
            extra["bank"] = bank
        got = k.store.stft_window(files, starts, frames, hop, n_fft, item_offsets=offsets, route_gains=gains, route_irs=irs, **extra)
        assert got.shape == (5, n_ch, 4 if output == "bank" else n_fft // 2 + 1, frames)
        for c in range(n_ch):
            keep = np.flatnonzero(irs[:, c] != NONE)
            row_of = np.searchsorted(offsets, keep, side="right") - 1
            offs = np.concatenate([[0], np.cumsum(np.bincount(row_of, minlength=5))]).astype(np.int64)
            want = k.store.stft_window(files[keep], starts[keep], frames, hop, n_fft, gains=gains[keep, c], item_offsets=offs,
                                       ir_index=irs[keep, c], **extra)
            if output == "complex":
                assert torch.equal(torch.view_as_real(got[:, c]), torch.view_as_real(want[:, 0])), (output, c)
            else:
                assert _same(got[:, c], want[:, 0]), (output, c)
        assert float(got.abs().max()) > 0.0
    assert k.store.route_info()["inverse_transforms"] > 0 and k.store.stft_ms() > 0.0


# ------------------------------------------------------------------ 6: the library's refusals
def _last_error(k):
    from mrcaudiocodec_amd import _lib
    return _lib.lib.mrc_last_error(k.h._h).decode()


def _raw(k, store=None, entry="decode", D=1, mix=0, ups=(1, 2), downs=(1, 3), n_ratios=None, zeros=16, rolloff=0.9, offsets=(0, 2),
         files=(0, 0), starts=(0, 9), ratio_of=(0, 1), route_gain=((1.0, 0.5), (0.25, 2.0)), route_ir=((0, -1), (NONE, 3)), window=16,
         channels=2, fmt=None, out="tensor", n_items=None, frames=None, hop=4):
    """the entry point itself -> (status, the pre-filled tensor)"""
    from mrcaudiocodec_amd import _lib
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)
    ups, downs, ratio_of, route_ir = arr(ups, np.int32), arr(downs, np.int32), arr(ratio_of, np.int32), arr(route_ir, np.int32)
    offsets, files, starts, route_gain = arr(offsets, np.int64), arr(files, np.int64), arr(starts, np.int64), arr(route_gain, np.float64)
    ptr = lambda a: None if a is None else a.ctypes.data
    n = (offsets.size - 1 if offsets is not None else 1) if n_items is None else n_items
    t = torch.full((max(n, 1), 16, 64), 77, dtype=torch.float64, device=torch.device("cuda", 0))
    head = ((store or k.store)._s, D, mix, (ups.size if ups is not None else 1) if n_ratios is None else n_ratios, ptr(ups), ptr(downs),
            zeros, rolloff, 0, None, None, n, ptr(offsets), ptr(files), ptr(starts), ptr(ratio_of), ptr(route_gain), ptr(route_ir))
    tail = (channels, _lib.MRC_WINDOW_F64 if fmt is None else fmt, t.data_ptr() if out == "tensor" else None, None)
    if entry == "decode":
        rc = _lib.lib.mrc_pac_store_decode_window_routed(*head, window, *tail)
    else:
        win = np.ones(16)
        rc = _lib.lib.mrc_pac_store_stft_window_routed(*head, 16, win.ctypes.data, (1 if window else 0) if frames is None else frames, hop, _lib.MRC_STFT_POWER, 0, None, *tail)
    return rc, t


def test_library_refusals_come_before_any_device_work(kitchen):
    from mrcaudiocodec_amd import _lib
    from mrcaudiocodec_amd.store import PacStore
    k = kitchen
    n_irs = len(LENGTHS)
    cases = [
        # this call's own
        (dict(channels=0), ("n_channels_out 0 is outside 1..16",)), (dict(channels=17), ("n_channels_out 17 is outside 1..16",)),
        (dict(mix=3), ("term 0: file 0 is stereo, the call asks for one channel",)),
        (dict(route_gain=None), ("route_gain or route_ir is NULL",)), (dict(route_ir=None), ("route_gain or route_ir is NULL",)),
        (dict(route_gain=((1.0, 0.5), (float("inf"), 2.0))), ("route_gain of term 1, channel 0 is not finite",)),
        (dict(route_ir=((0, -3), (NONE, 3))), ("route_ir of term 0, channel 1 = -3", "MRC_ROUTE_NONE (-2)")),
        (dict(route_ir=((0, -1), (n_irs, 3))), ("route_ir of term 1, channel 0 = %d" % n_irs, "bank of %d impulse responses" % n_irs)),
        (dict(window=(1 << 40) - 5, route_ir=((0, -1), (NONE, LENGTHS.index(B)))),
         ("window + the longest impulse response named - 1", "exceeds 2^40")),
        # the reverb call's, under this call's name
        (dict(D=3), ("rate_divisor 3",)), (dict(ratio_of=[0, 2]), ("ratio_of of term 1 = 2",)), (dict(mix=7), ("mix 7",)),
        (dict(files=[0, len(k.files)]), ("file[1]", "outside the store")), (dict(window=-1), ("window",)),
        (dict(fmt=9), ("format 9",)), (dict(out=None), ("out is NULL",)), (dict(offsets=[1, 2]), ("term_offset[0] = 1",)),
    ]
    for entry, fn in (("decode", "mrc_pac_store_decode_window_routed: "), ("stft", "mrc_pac_store_stft_window_routed: ")):
        for change, words in cases:
            if entry == "stft" and ("window" in change or "fmt" in change):
                continue                                     # (the STFT entry has no window, and formats of its own)
            rc, out = _raw(k, entry=entry, **change)
            text = _last_error(k)
            assert rc == _lib.MRC_ERR_INVALID and bool((out == 77).all()), (entry, change, rc, text)
            assert text.startswith(fn) and all(w in text for w in words), (entry, change, text)
    # the STFT entry's own bound: L = (n_frames - 1) hop + n_fft = 2^40 - 5 is allowed, L + Lpre is not
    rc, out = _raw(k, entry="stft", frames=(1 << 40) - 20, hop=1, route_ir=((0, -1), (NONE, LENGTHS.index(B))))
    text = _last_error(k)
    assert rc == _lib.MRC_ERR_INVALID and bool((out == 77).all()) and text.startswith("mrc_pac_store_stft_window_routed: ")
    assert "L + the longest impulse response named - 1" in text and "exceeds 2^40" in text
    with PacStore(k.h, k.files) as bare:                     # an index while the store has no bank
        rc, out = _raw(k, store=bare)
        text = _last_error(k)
        assert rc == _lib.MRC_ERR_INVALID and bool((out == 77).all())
        assert "route_ir of term 0, channel 0 = 0" in text and "has no impulse responses" in text
        rc, out = _raw(k, store=bare, route_ir=((-1, NONE), (NONE, -1)))
        assert rc == 0 and bool((out.reshape(-1)[:32] != 77).all())
    for change in (dict(offsets=[0], files=None, starts=None, ratio_of=None, route_gain=None, route_ir=None), dict(window=0)):
        for entry in ("decode", "stft"):
            rc, out = _raw(k, entry=entry, **change)
            assert rc == 0 and bool((out == 77).all()), (entry, change)
    rc, out = _raw(k)
    flat = out.reshape(-1)
    assert rc == 0 and bool((flat[:2 * 16] != 77).all()) and bool((flat[2 * 16:] == 77).all())
    # rows [1][2][16]: channel 1 of a row whose every route to it is absent is +0.0
    rc, out = _raw(k, route_ir=((0, NONE), (-1, NONE)))
    got = out.reshape(-1)[:32].reshape(2, 16)
    assert rc == 0 and bool(got[0].any()) and not bool(got[1].any()) and not bool(torch.signbit(got[1]).any())


# ------------------------------------------------------------------ 7: the command line
def test_cli_decodes_through_a_microphone_array(tmp_path, capsys):
    from mrcaudiocodec_amd import cli
    k = _kitchen_of("default")
    a, dst, one, npy, ir = (str(tmp_path / n) for n in ("a.pac", "x.wav", "one.wav", "mics.npy", "ir.npy"))
    with open(a, "wb") as fp:
        fp.write(k.files[0])
    mics = np.stack([RV.room(B + 7, 21), RV.room(B + 7, 22)])
    np.save(npy, mics)
    cli.main(["-d", a, dst, "--array-ir", npy, "--sample-rate", "16000", "--start", "100", "--samples", "3000"])
    got = open(dst, "rb").read()
    rate, n_ch, n, pcm = cli.read_wav_pcm(dst, 1)
    assert (rate, n_ch, n) == (16000, 2, 3000) and pcm[:, :n].any()
    for c in range(2):                                       # each channel is --ir with that response alone, on the mid
        np.save(ir, mics[c])
        cli.main(["-d", a, one, "--ir", ir, "--mix", "mid", "--sample-rate", "16000", "--start", "100", "--samples", "3000"])
        _, ch1, n1, want = cli.read_wav_pcm(one, 1)
        assert (ch1, n1) == (1, 3000) and np.array_equal(pcm[c, :n], want[0, :n1]), c
    assert got == cli.wav_bytes(pcm[:, :n], 16000)
    # ... and composes with what --ir composes with: a speed, band gains, an overlay (dry on every channel), all of them, and
    # the STFT of that row
    excerpt = ["--sample-rate", "16000", "--start", "100", "--samples", "3000"]
    overlay = ["--overlay", a, "--snr-db", "6", "--overlay-start", "700"]
    bands = ["--band-gains-db", "0-300:-inf,3400-8000:-6"]
    stft, mic = str(tmp_path / "x.npy"), str(tmp_path / "one.npy")
    for more in (["--speed", "11/10"], overlay, bands, ["--speed", "9/10"] + overlay + bands):
        cli.main(["-d", a, dst, "--array-ir", npy] + excerpt + more)
        _, n_ch, n, pcm = cli.read_wav_pcm(dst, 1)
        assert (n_ch, n) == (2, 3000) and pcm[:, :n].any()
        cli.main([a, stft, "--stft-energies", "--n-fft", "400", "--hop", "160", "--array-ir", npy] + excerpt + more)
        spectrum = np.load(stft)
        assert spectrum.shape == (2, 201, 17) and spectrum.any()
        for c in range(2):
            np.save(ir, mics[c])
            cli.main(["-d", a, one, "--ir", ir, "--mix", "mid"] + excerpt + more)
            _, ch1, n1, want = cli.read_wav_pcm(one, 1)
            assert (ch1, n1) == (1, 3000) and np.array_equal(pcm[c, :n], want[0, :n1]), (more, c)
            cli.main([a, mic, "--stft-energies", "--n-fft", "400", "--hop", "160", "--ir", ir, "--mix", "mid"] + excerpt + more)
            assert np.array_equal(spectrum[c], np.load(mic)[0]), (more, c)
    capsys.readouterr()
