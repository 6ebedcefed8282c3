"""
GPU tests of the rate ladder (mrc_encode_chained_ladder_pac / mrc_dev_encode_chained_ladder_pac): one chained call that
encodes the same streams at several target bit rates.  Output r must be, byte for byte and offset for offset, what the
one-rate chained call (mrc_encode_chained_stream_pac) gives on a handle whose target_bits_per_sample is rate r.
Streams are block-switched: their shapes come from the transient detector (transient.block_shape_array), as the
command line gets them, and hold all four block shapes.
"""
import ctypes as C

import numpy as np
import pytest

import chain_kit as kit
from chain_kit import HOP, handles_closed_after_module as _close_handles  # noqa: F401

pytestmark = pytest.mark.gpu

RATES = (1.0, 2.0, 2.86, 4.0, 6.5)


def _handle(tbps):
    """a handle at target_bits_per_sample = tbps (kept for the module: the one-rate reference calls)"""
    return kit.handle(target_bits_per_sample=tbps)


@pytest.fixture(scope="module")
def h():
    return _handle(2.86)


def _switched(h, hops, seed, mono=False):
    """int16 PCM codes [nCh][(hops + 1) * HOP] (zero prior hop) with bursts, and the detector's shapes [n][3] up to the last
    long block (Close() needs one)"""
    from mrcaudiocodec_amd import synth
    x, _ = synth.c4_transients(hops, seed=seed, period=7)
    tone = synth.c1_sine(hops, freq=440.0 + seed, amp=0.2)
    g = synth.c2_noise(hops, seed=seed + 1, sigma=0.03)[:len(x)]
    left = x + tone
    chans = [left] if mono else [left, 0.7 * x + 0.8 * tone + g]
    pcm = kit.to_pcm(np.stack(chans))
    return pcm, kit.shapes_to_last_long(h, pcm)


def _four_shapes(shapes):
    return len({(int(a), int(b)) for (_, a, b) in shapes}) == 4


def _check_equal(got, want, keys=("stream_offset", "reservoir_out", "reservoir_trace", "item_offset")):
    assert got["bytes"].tobytes() == want["bytes"].tobytes()
    assert got["total"] == want["total"]
    for k in keys:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k


def _singles(rates, left, right, shapes, **kw):
    return [_handle(r).encode_chained_pac(left, right, shapes, **kw) for r in rates]


@pytest.mark.parametrize("mono", [False, True])
@pytest.mark.parametrize("huff", [True, False])
def test_ladder_equals_one_call_per_rate(h, mono, huff):
    pcm, shapes = _switched(h, 40, seed=3, mono=mono)
    assert _four_shapes(shapes)
    right = None if mono else pcm[1][None]
    kw = dict(use_huffman=huff, num_samples=[len(shapes) * HOP], want_trace=True, want_items=True)
    got = h.encode_chained_pac_ladder(pcm[0][None], right, [shapes], RATES, **kw)
    want = _singles(RATES, pcm[0][None], right, [shapes], **kw)
    assert len(got) == len(RATES)
    for g, w in zip(got, want):
        _check_equal(g, w)
    sizes = [g["total"] for g in got]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]          # more bits per sample, more bytes


def _four_streams(h):
    """4 stereo streams of different lengths [4][stride] and their shape lists (the first one switched through all shapes)"""
    parts = [_switched(h, n, seed=s) for (n, s) in ((37, 11), (12, 12), (25, 13), (6, 14))]
    left, right, _ = kit.rows([p for (p, _) in parts])
    assert _four_shapes(parts[0][1])
    return left, right, [sh for (_, sh) in parts]


def test_streams_of_different_lengths_and_extreme_reservoirs(h):
    left, right, shapes = _four_streams(h)
    rates = (0.02, 2.86, 6.5)
    res_in = np.array([[0, -3000, 200000, 17], [5, 200000, -3000, 0], [-3000, 17, 0, 200000]], np.int32)
    kw = dict(num_samples=[len(sh) * HOP for sh in shapes], want_trace=True, want_items=True)
    got = h.encode_chained_pac_ladder(left, right, shapes, rates, reservoir_in=res_in, **kw)
    for r, rate in enumerate(rates):
        want = _handle(rate).encode_chained_pac(left, right, shapes, reservoir_in=res_in[r], **kw)
        _check_equal(got[r], want)


@pytest.mark.parametrize("slab", [7, 64])
def test_slabs_give_the_unslabbed_bytes(h, slab):
    left, right, shapes = _four_streams(h)
    long_pcm, long_shapes = _switched(h, 150, seed=21)
    assert len(long_shapes) > slab
    stride = max(left.shape[1], long_pcm.shape[1])
    L = np.zeros((5, stride), np.int16)
    Rt = np.zeros((5, stride), np.int16)
    L[:4, :left.shape[1]], Rt[:4, :left.shape[1]] = left, right
    L[4, :long_pcm.shape[1]], Rt[4, :long_pcm.shape[1]] = long_pcm
    shapes = shapes + [long_shapes]
    rates = (1.0, 2.86, 4.0)
    res_in = np.arange(15, dtype=np.int32).reshape(3, 5) * 7 - 20
    kw = dict(num_samples=[len(sh) * HOP for sh in shapes], want_trace=True, want_items=True, reservoir_in=res_in)
    h.set_option(6, 0)
    try:
        whole = h.encode_chained_pac_ladder(L, Rt, shapes, rates, **kw)
        h.set_option(6, slab)
        got = h.encode_chained_pac_ladder(L, Rt, shapes, rates, **kw)
    finally:
        h.set_option(6, 131072)
    for r, rate in enumerate(rates):
        _check_equal(got[r], whole[r])
        want = _handle(rate).encode_chained_pac(L, Rt, shapes, **dict(kw, reservoir_in=res_in[r]))
        _check_equal(got[r], want)


def test_resident_entry_and_float_input(h):
    torch = pytest.importorskip("torch")
    from mrcaudiocodec_amd import synth
    left, right, shapes = _four_streams(h)
    rates = (1.5, 2.86, 5.0)
    kw = dict(num_samples=[len(sh) * HOP for sh in shapes], want_items=True, want_trace=True)
    host = h.encode_chained_pac_ladder(left, right, shapes, rates, **kw)
    fl = h.encode_chained_pac_ladder(synth.pcm_to_float(left), synth.pcm_to_float(right), shapes, rates, **kw)
    for a, b in zip(host, fl):
        _check_equal(b, a)
    dev = torch.device("cuda", 0)
    dl, dr = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    start, _, a, b = h._chain_schedule(shapes)
    bound = h.chain_out_bound(start, a, b, True, True, 2)
    outs = [torch.full((bound,), 0xA5, dtype=torch.uint8, device=dev) for _ in rates]
    torch.cuda.synchronize(dev)
    res = h.encode_chained_pac_ladder(None, None, shapes, rates,
                                      device=(dl.data_ptr(), dr.data_ptr(), 1, left.shape[1], [o.data_ptr() for o in outs],
                                              [bound] * len(rates)),
                                      stream=torch.cuda.current_stream(dev).cuda_stream, **kw)
    for r in range(len(rates)):
        assert res[r]["bytes"] is None
        assert outs[r][:res[r]["total"]].cpu().numpy().tobytes() == host[r]["bytes"].tobytes()
        for k in ("stream_offset", "item_offset", "reservoir_out", "reservoir_trace"):
            assert np.array_equal(res[r][k], host[r][k]), k


def test_rate_handling(h):
    pcm, shapes = _switched(h, 30, seed=5)
    kw = dict(num_samples=[len(shapes) * HOP], want_trace=True, want_items=True)
    before = h.encode_chained_pac(pcm[0][None], pcm[1][None], [shapes], **kw)
    one = h.encode_chained_pac_ladder(pcm[0][None], pcm[1][None], [shapes], [4.0], **kw)
    assert len(one) == 1
    _check_equal(one[0], _handle(4.0).encode_chained_pac(pcm[0][None], pcm[1][None], [shapes], **kw))
    assert h.cfg.target_bits_per_sample == 2.86
    _check_equal(h.encode_chained_pac(pcm[0][None], pcm[1][None], [shapes], **kw), before)
    dup = h.encode_chained_pac_ladder(pcm[0][None], pcm[1][None], [shapes], [3.0, 2.86, 3.0, 2.86], **kw)
    _check_equal(dup[0], dup[2])
    _check_equal(dup[1], dup[3])
    _check_equal(dup[1], before)


def _raw_ladder(h, pcm, shapes, rates, outs, caps, lib_fn="mrc_encode_chained_ladder_pac"):
    """the C entry point with explicit arguments: -> (rc, total_bytes [R])"""
    from mrcaudiocodec_amd._lib import lib
    start, off, a, b = h._chain_schedule([shapes])
    R = len(rates)
    rates = np.ascontiguousarray(rates, dtype=np.float64)
    left, right = np.ascontiguousarray(pcm[0][None]), np.ascontiguousarray(pcm[1][None])
    ptrs = (C.c_void_p * max(R, 1))(*[(o.ctypes.data if o is not None else None) for o in outs])
    caps = np.ascontiguousarray(caps, dtype=np.int64)
    s_off = np.zeros((max(R, 1), 2), np.int64)
    total = np.zeros(max(R, 1), np.int64)
    ns = np.array([len(shapes) * HOP], np.uint32)
    rc = getattr(lib, lib_fn)(h._h, R, rates.ctypes.data, 1, left.ctypes.data, right.ctypes.data, 1, left.shape[1],
                              start.ctypes.data, off.ctypes.data, a.ctypes.data, b.ctypes.data, None, 1, 1, ns.ctypes.data,
                              C.cast(ptrs, C.c_void_p), caps.ctypes.data, s_off.ctypes.data, None, None, None,
                              total.ctypes.data)
    return rc, total


def test_refusals_and_small_buffers(h):
    from mrcaudiocodec_amd._lib import lib, MRC_ERR_INVALID, MRC_ERR_NOMEM
    pcm, shapes = _switched(h, 12, seed=8)
    start, _, a, b = h._chain_schedule([shapes])
    bound = h.chain_out_bound(start, a, b, True, True, 2)
    buf = lambda: np.zeros(bound, np.uint8)
    for rates in ([], [2.0] * 17):                                    # n_rates outside 1..16
        assert _raw_ladder(h, pcm, shapes, rates, [buf() for _ in rates], [bound] * len(rates))[0] == MRC_ERR_INVALID
        assert b"n_rates" in lib.mrc_last_error(h._h)
    for bad in (float("nan"), float("inf"), 0.0, -1.0, 64.5):         # rates not finite or outside (0, 64]
        assert _raw_ladder(h, pcm, shapes, [2.0, bad], [buf(), buf()], [bound] * 2)[0] == MRC_ERR_INVALID
        assert b"target_bits_per_sample[1]" in lib.mrc_last_error(h._h)
    assert _raw_ladder(h, pcm, shapes, [2.0, 64.0], [buf(), None], [bound] * 2)[0] == MRC_ERR_INVALID   # a NULL out[r]
    assert b"out[1]" in lib.mrc_last_error(h._h)
    h.set_option(5, 1)                                                # MRC_OPT_SENSITIVITY
    try:
        assert _raw_ladder(h, pcm, shapes, [2.0, 3.0], [buf(), buf()], [bound] * 2)[0] == MRC_ERR_INVALID
        assert b"MRC_OPT_SENSITIVITY" in lib.mrc_last_error(h._h)
    finally:
        h.set_option(5, 0)
    # one buffer too small: MRC_ERR_NOMEM, every size reported; a second call with those sizes succeeds
    rates = [1.0, 2.86, 6.5]
    rc, total = _raw_ladder(h, pcm, shapes, rates, [buf(), buf(), buf()], [bound, 100, bound])
    assert rc == MRC_ERR_NOMEM and (total > 100).all() and total[0] < total[1] < total[2]
    outs = [np.zeros(int(t), np.uint8) for t in total]
    rc2, total2 = _raw_ladder(h, pcm, shapes, rates, outs, total)
    assert rc2 == 0 and np.array_equal(total2, total)
    want = _singles(rates, pcm[0][None], pcm[1][None], [shapes], num_samples=[len(shapes) * HOP])
    for o, w in zip(outs, want):
        assert o.tobytes() == w["bytes"].tobytes()
    # nothing of the ladder is served by mrc_chain_fetch_output, even after a one-rate call held output
    h.encode_chained_pac(pcm[0][None], pcm[1][None], [shapes])
    _raw_ladder(h, pcm, shapes, rates, outs, total)
    t = np.zeros(1, np.int64)
    assert lib.mrc_chain_fetch_output(h._h, buf().ctypes.data, bound, t.ctypes.data) == MRC_ERR_INVALID


def _snr(ref, got):
    n = min(ref.shape[1], got.shape[1])
    ref, got = ref[:, :n].astype(np.float64), got[:, :n].astype(np.float64)
    return 10 * np.log10((ref ** 2).sum() / max(((got - ref) ** 2).sum(), 1e-30))


@pytest.mark.parametrize("mono", [False, True])
def test_every_rate_decodes(h, mono):
    from mrcaudiocodec_amd import pacfile
    pcm, shapes = _switched(h, 30, seed=9, mono=mono)
    rates = (1.0, 2.86, 6.5)
    files = pacfile.encode_stream_ladder(h, pcm if not mono else pcm[0], shapes, rates)
    snr = []
    for data in files:
        dec = h.decode_pac_pcm16(data, interleaved=False)[0]
        assert dec.shape[0] == pcm.shape[0]
        snr.append(_snr(pcm[:, HOP:HOP + len(shapes) * HOP], dec))
    assert snr[2] > snr[0] and snr[2] > 10, snr


def test_ladder_memory_stays_within_twice_one_rate():
    """2^17-hop stereo stream, slabs of 65 536 blocks: an 8-rate ladder's device memory stays under 2x the one-rate call's"""
    torch = pytest.importorskip("torch")
    from mrcaudiocodec_amd import Handle
    dev = torch.device("cuda", 0)
    hops = 1 << 17
    rng = np.random.default_rng(1)
    pcm = np.zeros((2, (hops + 1) * HOP), np.int16)
    pcm[:, HOP:] = np.clip(np.rint(rng.normal(0, 0.05 * 32767, (2, hops * HOP))), -32767, 32767)
    shapes = np.stack([np.arange(hops, dtype=np.int64) * HOP, np.full(hops, HOP, np.int64), np.full(hops, HOP, np.int64)], axis=1)
    used = []
    for rates in (None, (1.0, 1.5, 2.0, 2.86, 3.5, 4.0, 5.0, 6.5)):
        torch.cuda.synchronize(dev)
        free0, _ = torch.cuda.mem_get_info(dev)
        hd = Handle(device_id=0)
        try:
            hd.set_option(6, 65536)
            if rates is None:
                r = hd.encode_chained_pac(pcm[0][None], pcm[1][None], [shapes], num_samples=[hops * HOP])
            else:
                r = hd.encode_chained_pac_ladder(pcm[0][None], pcm[1][None], [shapes], rates, num_samples=[hops * HOP])
            torch.cuda.synchronize(dev)
            free1, _ = torch.cuda.mem_get_info(dev)
            used.append(free0 - free1)
        finally:
            hd.close()
        del r
    assert used[1] < 2 * used[0] and used[1] < 8e9, [u / 1e9 for u in used]


@pytest.mark.parametrize("mono", [False, True])
def test_cli_ladder(h, tmp_path, mono):
    from mrcaudiocodec_amd import cli
    pcm, _ = _switched(h, 25, seed=17, mono=mono)
    src = kit.write_wav(tmp_path / "in.wav", pcm[:, HOP:])
    cli.main([src, str(tmp_path / "plain.pac")])
    cli.main([src, str(tmp_path / "out_{bps}.pac"), "--bits-per-sample", "2,2.86,4"])
    files = {v: (tmp_path / ("out_%s.pac" % v)).read_bytes() for v in ("2", "2.86", "4")}
    assert files["2.86"] == (tmp_path / "plain.pac").read_bytes()
    assert len(files["2"]) < len(files["2.86"]) < len(files["4"])
    cli.main([src, str(tmp_path / "one.pac"), "--bits-per-sample", "4"])
    assert (tmp_path / "one.pac").read_bytes() == files["4"]
    for v, data in files.items():
        dec = h.decode_pac_pcm16(data, interleaved=False)[0]
        assert dec.shape[0] == pcm.shape[0], v
