"""
GPU tests of the store's rational-rate windows (mrc_pac_store_decode_window_resampled, PacStore.decode_window(resample=), cli -d
--sample-rate): the float64 windows equal, bit for bit, the NumPy restatement of the header's fold over the store's own
intermediate windows (tests/resample_restatement.py) -- for every rate divisor, mix, tile edge of the kernel's workgroup and
start around every block boundary, before the file, across its end and past it; the other two formats as conversions of the
call's own float64 window; the channel map; independence of order, company and slab size; that work follows the
intermediate spans; extreme starts; the library's refusals; the command line.  Files: the five-hop default-setting stereo file
of tests/test_gpu_store_reduced.py and the kit's files at setting B (tests/settings_kit.py): the smallest that hold every
block shape and a non-joint last block.
"""
import struct

import numpy as np
import pytest

import chain_kit as kit
from chain_kit import handles_closed_after_module  # noqa: F401
import resample_restatement as RS
from oracle import decode as odec

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIDS = ("default", "B")
SLAB_OPTION, SLAB_DEFAULT = 7, 1 << 24
ROLLOFF = 0.9475
# (rate_divisor, up, down, zeros)
CASES = ((1, 1, 3, 16), (2, 2, 3, 16), (1, 3, 2, 16), (1, 160, 441, 16), (4, 8, 1, 16), (1, 1, 3, 6))
MIXES = (None, "mid", "left")
WINDOWS = (1, 255, 256, 257, 700)                    # the workgroup's tile of 256 outputs: below, at and above its edge

_KITCHENS = {}


@pytest.fixture(scope="module", params=SIDS)
def kitchen(request):
    from test_gpu_store_reduced import _Kitchen
    sid = request.param
    if sid not in _KITCHENS:
        _KITCHENS[sid] = _Kitchen(sid)
    return _KITCHENS[sid]


@pytest.fixture(scope="module", autouse=True)
def stores_closed_after_module():
    yield
    for k in _KITCHENS.values():
        k.store.close()
    _KITCHENS.clear()


def _w(up, down, zeros):
    from mrcaudiocodec_amd.store import resample_taps
    return resample_taps(up, down, zeros, ROLLOFF)[0]


def _items(k, D, up, down, zeros, window):
    """(file, start): output starts at every intermediate block boundary b mapped to output samples, floor(b up / down), and
    one either side; -37; the start whose span straddles the file's end; one wholly past the end"""
    W, out, past = _w(up, down, zeros), [], []
    for f in range(len(k.files)):
        n = int(k.index[f]["n_samples"]) // D
        out += [(f, b * up // down + d) for b in k.boundaries(f, D) for d in (-1, 0, 1)]
        out += [(f, -37), (f, -(-n * up // down) - window // 2)]
        beyond = -(-(n + W) * up // down) + 1
        assert RS.span(beyond, window, up, down, W)[0] >= n
        past.append((f, beyond))
    return out + past, len(past)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int64), b.view(np.int64))


def _raw(k, D, mix, up, down, zeros, rolloff, items, window, channels, dtype):
    """the entry point itself -> (status, tensor)"""
    from mrcaudiocodec_amd import _lib
    from mrcaudiocodec_amd.store import _formats
    files = np.ascontiguousarray([f for f, _ in items], dtype=np.int64)
    starts = np.ascontiguousarray([s for _, s in items], dtype=np.int64)
    out = torch.full((len(items), channels, window), 77, dtype=dtype, device=torch.device("cuda", 0))
    rc = _lib.lib.mrc_pac_store_decode_window_resampled(k.store._s, D, mix, up, down, zeros, rolloff, len(items), files.ctypes.data,
                                                        starts.ctypes.data, window, channels, _formats()[dtype], out.data_ptr(), None)
    return rc, out


# ------------------------------------------------------------------ 1: float64 equals the restatement, bit for bit
@pytest.mark.parametrize("mix", MIXES)
@pytest.mark.parametrize("D,up,down,zeros", CASES)
def test_f64_equals_the_restatement_bit_for_bit(kitchen, D, up, down, zeros, mix):
    k = kitchen
    channels = 2 if mix is None else None
    for window in WINDOWS:
        items, n_past = _items(k, D, up, down, zeros, window)
        files, starts = zip(*items)
        got = k.store.decode_window(files, starts, window, channels=channels, dtype=torch.float64, rate_divisor=D, mix=mix,
                                    resample=(up, down, zeros, ROLLOFF)).cpu().numpy()
        want = RS.restate(k.store, files, starts, window, up, down, zeros, ROLLOFF, D, mix, channels)
        assert got.shape == (len(items), 2 if mix is None else 1, window)
        assert _same_bits(got, want), (k.sid, D, up, down, zeros, mix, window, np.abs(got - want).max())
        assert np.abs(got[:-n_past]).max() > 1e-3                # (signal, not silence)
        tail = got[-n_past:]                                     # wholly past the end: +0.0
        assert not tail.any() and not np.signbit(tail).any()


def _default_kitchen():
    from test_gpu_store_reduced import _Kitchen
    return _KITCHENS.get("default") or _KITCHENS.setdefault("default", _Kitchen("default"))


def test_resampled_signal_is_the_signal():
    """not only the restatement's bits: the 16 kHz window of the default file (two tones at 1 and 5.2 kHz over weaker noise) is
    its half-rate window read at 3 / 2 sample steps, up to the noise above 8 kHz that the filter takes out, and a ratio of 1
    after reduction is the call without resample"""
    k = _default_kitchen()
    n = int(k.index[0]["n_samples"]) // 2
    y = k.store.decode_window([0], [0], n, dtype=torch.float64, rate_divisor=2)[0].cpu().numpy()
    n_out = int(k.store.n_samples_resampled(2, 3, 2)[0])
    assert n_out == -(-n * 2 // 3)
    v = k.store.decode_window([0], [0], n_out, dtype=torch.float64, rate_divisor=2, resample=(2, 3))[0].cpu().numpy()
    even = v[:, 0::2][:, :n // 3]                                # output 2 i sits on intermediate sample 3 i: phase 0
    at = y[:, 0:3 * even.shape[1]:3]
    corr = np.sum(even * at) / np.sqrt(np.sum(even * even) * np.sum(at * at))
    print("correlation of the 16 kHz window with the half-rate window at the same times: %.4f" % corr)
    assert corr > 0.9
    assert 0.5 * np.abs(y).max() < np.abs(v).max() < 1.5 * np.abs(y).max()
    same = k.store.decode_window([0], [5], 300, dtype=torch.float64, rate_divisor=2, resample=(7, 7))
    assert torch.equal(same, k.store.decode_window([0], [5], 300, dtype=torch.float64, rate_divisor=2))


# ------------------------------------------------------------------ 2: the other formats, the channel map
@pytest.mark.parametrize("D,up,down,zeros", [(2, 2, 3, 16), (1, 160, 441, 16)])
def test_formats_are_conversions_of_the_f64_window(kitchen, D, up, down, zeros):
    k = kitchen
    window = 257
    items, _ = _items(k, D, up, down, zeros, window)
    files, starts = zip(*items)
    kw = dict(channels=2, rate_divisor=D, resample=(up, down, zeros, ROLLOFF))
    f64 = k.store.decode_window(files, starts, window, dtype=torch.float64, **kw).cpu().numpy()
    i16 = k.store.decode_window(files, starts, window, **kw)
    f32 = k.store.decode_window(files, starts, window, dtype=torch.float32, **kw)
    assert i16.dtype == torch.int16 and f32.dtype == torch.float32 and f64.any()
    assert np.array_equal(i16.cpu().numpy(), odec.pcm16(f64))
    assert np.array_equal(f32.cpu().numpy(), f64.astype(np.float32))
    mono = [i for i, (f, _) in enumerate(items) if k.index[f]["n_channels"] == 1]
    if mono:                                                     # a mono file fills both channels; alone, it has one
        assert _same_bits(f64[mono][:, 0], f64[mono][:, 1]) and f64[mono].any()
        alone = k.store.decode_window([files[i] for i in mono], [starts[i] for i in mono], window, dtype=torch.float64,
                                      rate_divisor=D, resample=(up, down, zeros, ROLLOFF))
        assert tuple(alone.shape) == (len(mono), 1, window) and _same_bits(alone.cpu().numpy()[:, 0], f64[mono][:, 0])


def test_stereo_file_in_a_one_channel_call_is_refused(kitchen):
    from mrcaudiocodec_amd import MrcError
    k = kitchen
    out = torch.full((1, 1, 32), 12345, dtype=torch.int16, device=torch.device("cuda", 0))
    with pytest.raises(MrcError, match=r"mrc_pac_store_decode_window_resampled: item 0: file 0 is stereo") as e:
        k.store.decode_window([0], [0], 32, channels=1, out=out, rate_divisor=2, resample=(2, 3))
    assert e.value.code == -1 and bool((out == 12345).all())
    one = k.store.decode_window([0], [0], 32, channels=1, out=out, rate_divisor=2, resample=(2, 3), mix="right")
    assert one is out and bool((out != 12345).any())


# ------------------------------------------------------------------ 3: independence
@pytest.mark.parametrize("D,up,down,zeros,mix", [(2, 2, 3, 16, None), (1, 160, 441, 16, "mid"), (1, 1, 3, 6, None)])
def test_result_does_not_depend_on_order_company_or_slabs(kitchen, D, up, down, zeros, mix):
    k = kitchen
    window = 300
    items, _ = _items(k, D, up, down, zeros, window)
    files, starts = map(np.array, zip(*items))
    kw = dict(channels=2 if mix is None else None, dtype=torch.float64, rate_divisor=D, mix=mix, resample=(up, down, zeros, ROLLOFF))
    base = k.store.decode_window(files, starts, window, **kw)
    assert k.store.stats()["slabs"] == 1
    same = lambda a, b: torch.equal(a, b) and torch.equal(torch.signbit(a), torch.signbit(b))
    assert same(k.store.decode_window(files[::-1].copy(), starts[::-1].copy(), window, **kw).flip(0), base)
    for i in range(0, len(items), 4):
        assert same(k.store.decode_window(files[i:i + 1], starts[i:i + 1], window, **kw)[0], base[i])
    try:
        k.h.set_option(SLAB_OPTION, 1)                           # no two spans fit: every item is its own slab
        got = k.store.decode_window(files, starts, window, **kw)
        assert k.store.stats()["slabs"] == len(items) and same(got, base)
        span = RS.span_bound(window, up // np.gcd(up, down), down // np.gcd(up, down), _w(up, down, zeros))
        k.h.set_option(SLAB_OPTION, 3 * span)                    # the rule counts plane samples: three spans per slab
        got = k.store.decode_window(files, starts, window, **kw)
        assert k.store.stats()["slabs"] == (len(items) + 2) // 3 and same(got, base)
    finally:
        k.h.set_option(SLAB_OPTION, SLAB_DEFAULT)


# ------------------------------------------------------------------ 4: work follows the windows
@pytest.mark.parametrize("D,up,down,zeros,mix", [(2, 2, 3, 16, None), (1, 1, 3, 16, "left"), (4, 8, 1, 16, "mid")])
def test_chunks_parsed_are_those_of_the_intermediate_spans(kitchen, D, up, down, zeros, mix):
    k = kitchen
    W = _w(up, down, zeros)
    seen, total, cases = set(), 0, []
    for window in (1, 300):
        items, n_past = _items(k, D, up, down, zeros, window)
        cases += [(f, s, window) for (f, s) in items[:-n_past:3] + items[-n_past:]]
    kw = dict(rate_divisor=D, mix=mix)
    for (f, s, w) in cases:
        k.store.decode_window([f], [s], w, resample=(up, down, zeros, ROLLOFF), **kw)
        got = k.store.stats()
        first, last = RS.span(s, w, up, down, W)
        k.store.decode_window([f], [first], last - first + 1, **kw)
        want = k.store.stats()
        assert got["chunks_parsed"] == want["chunks_parsed"], (k.sid, f, s, w)
        assert got["decode_launches"] == want["decode_launches"] and (got["decode_launches"] == 0) == (want["chunks_parsed"] == 0)
        seen.add(want["chunks_parsed"])
        total += want["chunks_parsed"] if w == 300 else 0
    assert len(seen) > 2 and 0 in seen
    files, starts = zip(*[(f, s) for (f, s, w) in cases if w == 300])
    k.store.decode_window(files, starts, 300, resample=(up, down, zeros, ROLLOFF), **kw)     # together: the sum
    assert k.store.stats()["chunks_parsed"] == total
    assert k.store.stats()["ms"]["window_out"] > 0.0


# ------------------------------------------------------------------ 5: extreme starts
def test_extreme_starts_give_zeros_and_no_error(kitchen):
    k = kitchen
    for (D, up, down) in ((1, 160, 441), (2, 2, 3), (1, 8, 1), (1, 1, 8)):
        for start in (1 << 39, -(1 << 39), 1 << 62, -(1 << 62)):
            for dtype in (torch.float64, torch.int16):
                got = k.store.decode_window([0, 0], [start, 0], 300, dtype=dtype, rate_divisor=D, resample=(up, down))
                assert not bool(got[0].any()) and bool(got[1].any())
                if dtype == torch.float64:
                    assert not bool(torch.signbit(got[0]).any())
        got = k.store.decode_window([0], [1 << 39], 300, dtype=torch.float64, rate_divisor=D, resample=(up, down))
        assert not bool(got.any()) and k.store.stats()["chunks_parsed"] == 0


# ------------------------------------------------------------------ 6: the library's refusals
def test_library_refusals_come_before_any_device_work(kitchen):
    from mrcaudiocodec_amd import _lib
    k = kitchen
    E, MID = _lib.MRC_MIX_EACH, _lib.MRC_MIX_MID
    fn = "mrc_pac_store_decode_window_resampled: "
    for (args, channels, words) in (
            ((1, E, 1, 9, 16, 0.9), 2, ("down 9", "8 * up")), ((1, E, 9, 1, 16, 0.9), 2, ("up 9", "8 * down")),
            ((1, E, 0, 3, 16, 0.9), 2, ("up 0",)), ((1, E, 3, 3, 16, 0.9), 2, ("up / down is 1",)),
            ((1, E, 1025, 1024, 16, 0.9), 2, ("up 1025",)), ((1, E, 2, 3, 0, 0.9), 2, ("zeros 0",)),
            ((1, E, 2, 3, 65, 0.9), 2, ("zeros 65",)), ((1, E, 2, 3, 16, 0.25), 2, ("rolloff",)),
            ((1, E, 2, 3, 16, 1.5), 2, ("rolloff",)), ((1, 7, 2, 3, 16, 0.9), 2, ("mix 7", "MRC_MIX_EACH (3)")),
            ((1, -1, 2, 3, 16, 0.9), 2, ("mix -1",)), ((1, MID, 2, 3, 16, 0.9), 2, ("n_channels_out must be 1",)),
            ((3, E, 2, 3, 16, 0.9), 2, ("rate_divisor 3",)), ((0, MID, 2, 3, 16, 0.9), 1, ("rate_divisor 0",)),
            ((2, E, 2, 3, 16, 0.9), 1, ("item 0: file 0 is stereo",))):
        rc, out = _raw(k, *args, [(0, 0)], 16, channels, torch.float64)
        text = _lib.lib.mrc_last_error(k.h._h).decode()
        assert rc == _lib.MRC_ERR_INVALID and bool((out == 77).all()), (args, text)
        assert text.startswith(fn) and all(w in text for w in words), (args, text)
    for (items, window, words) in (([(len(k.files), 0)], 16, "outside the store"), ([(0, 0)], -1, "window"), ([(0, 0)], (1 << 40) + 1, "window")):
        files = np.array([f for f, _ in items], np.int64)
        starts = np.array([s for _, s in items], np.int64)
        out = torch.full((1, 2, 16), 77, dtype=torch.float64, device=torch.device("cuda", 0))      # (the window refusals come first)
        rc = _lib.lib.mrc_pac_store_decode_window_resampled(k.store._s, 1, E, 2, 3, 16, 0.9, len(items), files.ctypes.data,
                                                            starts.ctypes.data, window, 2, _lib.MRC_WINDOW_F64, out.data_ptr(), None)
        assert rc == _lib.MRC_ERR_INVALID and words in _lib.lib.mrc_last_error(k.h._h).decode() and bool((out == 77).all())
    rc, out = _raw(k, 1, E, 2, 3, 16, 0.9, [], 16, 2, torch.float64)                     # nothing to do: MRC_OK, nothing written
    assert rc == 0


# ------------------------------------------------------------------ 7: the command line
def test_cli_decodes_at_16_khz(tmp_path):
    from mrcaudiocodec_amd import cli
    k = _default_kitchen()
    src, dst = str(tmp_path / "x.pac"), str(tmp_path / "x.wav")
    with open(src, "wb") as f:
        f.write(k.files[0])
    n = int(k.store.n_samples_resampled(2, 3, 2)[0])
    assert n == -(-(int(k.index[0]["n_samples"]) // 2) * 2 // 3)
    want = k.store.decode_window([0], [0], n, dtype=torch.int16, rate_divisor=2, resample=(2, 3))[0].cpu().numpy()
    cli.main(["-d", src, dst, "--sample-rate", "16000"])
    wav = open(dst, "rb").read()
    assert struct.unpack("<L", wav[24:28])[0] == 16000 and struct.unpack("<H", wav[22:24])[0] == 2
    assert wav == cli.wav_bytes(want, 16000) and want.any()
    cli.main(["-d", src, dst, "--sample-rate", "22050", "--mix", "mid", "--start", "100", "--samples", "300"])
    want_mid = k.store.decode_window([0], [100], 300, rate_divisor=2, mix="mid", resample=(147, 160))[0].cpu().numpy()
    assert open(dst, "rb").read() == cli.wav_bytes(want_mid, 22050) and want_mid.shape == (1, 300)
    cli.main(["-d", src, dst, "--sample-rate", "24000"])                                # a divisor alone gives the rate
    assert open(dst, "rb").read() == cli.wav_bytes(k.store.decode_window([0], [0], int(k.index[0]["n_samples"]) // 2,
                                                                         rate_divisor=2)[0].cpu().numpy(), 24000)
