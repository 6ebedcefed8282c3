"""
GPU tests of what a Handle owns and how it goes away: every device buffer, page-locked buffer, event and stream of the
handle is a member that frees itself when mrc_destroy deletes the handle (mrc_handle.hpp).  Nothing here can see a leak; what
the tests see is that closing a handle, growing a buffer under live ones and a create that fails leave every later result
as it was.  Every comparison of results is equality; times need only be finite and not negative.

The inputs are the smallest each path takes: 4 hops of seeded noise with a burst (one stereo stream, one mono), the block
schedule of that burst (long, start, 7 short, stop, long), and 5 long frames for the pipelined calls, whose chunks of one
frame go once round the kLanes = 4 chunk buffers and into the first again.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HOP, SHORT = 1024, 128
RATES = (2.0, 4.0)
OPT_SENSITIVITY, OPT_SLAB_BLOCKS, SLAB_DEFAULT = 5, 6, 131072
# (offset, a, b): long | start | 7 short | stop | long -- 4 hops behind the prior hop
SHAPES = np.array([(0, HOP, HOP), (HOP, HOP, SHORT)] + [(2 * HOP + k * SHORT, SHORT, SHORT) for k in range(7)] +
                  [(2 * HOP + 7 * SHORT, SHORT, HOP), (3 * HOP, HOP, HOP)], np.int64)
NS = int(SHAPES[:, 2].sum())                              # the files' sample count: 4 hops


def _pcm(hops, seed, nch):
    """int16 [nch][(hops + 1) * HOP]: a zero prior hop, noise, a burst at the start of the second hop"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 0.02 * 32767, (nch, (hops + 1) * HOP))
    x[:, 2 * HOP:2 * HOP + SHORT] = rng.normal(0.0, 0.4 * 32767, (nch, SHORT))
    pcm = np.clip(np.rint(x), -32767, 32767).astype(np.int16)
    pcm[:, :HOP] = 0
    return pcm


STEREO, MONO, FRAMES = _pcm(4, 11, 2), _pcm(4, 12, 1), _pcm(5, 13, 2)


def _blocks(x, n):
    """n long blocks [n][2 * HOP] of the float stream x, the first n - 1 hops over and over"""
    hops = len(x) // HOP - 1
    return np.stack([x[(i % hops) * HOP:(i % hops) * HOP + 2 * HOP] for i in range(n)])


def _files(res):
    return [r["data"] for r in res]


def _chained(r):
    return {"bytes": r["bytes"].tobytes(), "stream_offset": r["stream_offset"], "reservoir_out": r["reservoir_out"]}


def _measured(res):
    return [{k: v for k, v in r.items()} for r in res]


def _run_all(h):
    """once every family of calls that owns buffers or events -> (results, times)"""
    from mrcaudiocodec_amd import synth, transient
    out, ms = {}, {}
    fl, fr = synth.pcm_to_float(STEREO[0]), synth.pcm_to_float(STEREO[1])
    for n in (1, 65):                                     # the small-batch path | the staged path
        out["mono", n] = h.encode_mono(_blocks(fl, n), HOP, HOP, want_mdct=True)
        out["joint", n] = h.encode_joint(_blocks(fl, n), _blocks(fr, n), HOP, HOP, want_mdct=True)
    mixed = SHAPES[[0, 1, 2, 9]]
    cut = lambda x: [x[o:o + a + b] for o, a, b in mixed]
    out["blocks mono"] = h.encode_blocks(cut(fl), mixed[:, 1], mixed[:, 2])
    out["blocks joint"] = h.encode_blocks(cut(fl), mixed[:, 1], mixed[:, 2], right=cut(fr))
    # chunks of one frame: five chunks over four lanes
    out["pcm16 joint"] = h.encode_stream_pcm16(FRAMES[0], FRAMES[1], chunk_frames=1)
    out["pcm16 mono"] = h.encode_stream_pcm16(FRAMES[0], chunk_frames=1)
    out["pcm16 pac joint"] = h.encode_stream_pcm16_pac(FRAMES[0], FRAMES[1], chunk_frames=1)
    out["pcm16 pac mono"] = h.encode_stream_pcm16_pac(FRAMES[0], use_huffman=False, chunk_frames=1)
    for name, left, right in (("stereo", STEREO[0:1], STEREO[1:2]), ("mono", MONO, None)):
        args = (left, right, [SHAPES])
        out["chained", name] = _chained(h.encode_chained_pac(*args, num_samples=[NS]))
        ms["chain", name] = h.chain_ms()
        out["ladder", name] = [_chained(r) for r in h.encode_chained_pac_ladder(*args, RATES, num_samples=[NS])]
        out["target", name] = _measured(h.encode_chained_pac_target_nmr(*args, RATES, -3.0, num_samples=[NS]))
        ms["target", name] = h.target_ms()
        out["vbr", name] = _measured(h.encode_vbr_nmr_pac(*args, 0.0, num_samples=[NS]))
        ms["vbr", name] = h.vbr_ms()
        size = len(out["vbr", name][0]["data"])
        out["vbr size", name] = _measured(h.encode_vbr_size_pac(*args, [size], -12.0, 3.0, 8, num_samples=[NS]))
        ms["vbr size", name] = h.vbr_size_ms()
    files = [out["chained", "stereo"]["bytes"], out["chained", "mono"]["bytes"]]
    sources = [np.ascontiguousarray(STEREO[:, HOP:]), np.ascontiguousarray(MONO[:, HOP:])]
    out["decode"] = h.decode_pac_pcm16(files)
    ms["decode"] = h.decode_ms()
    out["nmr"] = h.pac_nmr(files, sources, detail=True)
    ms["nmr"] = h.nmr_ms()
    out["peaks"] = h.transient_peaks(STEREO, transient.design_sos(48000))
    h.set_option(OPT_SENSITIVITY, 1)
    out["sens mono"] = h.encode_mono(_blocks(fl, 3), HOP, HOP)
    out["sens joint"] = h.encode_joint(_blocks(fl, 1), _blocks(fr, 1), HOP, HOP)
    out["sensitivity"] = h.sensitivity()
    h.set_option(OPT_SENSITIVITY, 0)
    h.set_timing(True)
    out["timed mono"] = h.encode_mono(_blocks(fl, 65), HOP, HOP)
    ms["kernel", 65], ms["stage", 65] = h.kernel_ms(), h.stage_ms()
    out["timed joint"] = h.encode_joint(_blocks(fl, 1), _blocks(fr, 1), HOP, HOP)
    ms["kernel", 1], ms["stage", 1] = h.kernel_ms(), h.stage_ms()
    h.set_timing(False)
    return out, ms


def _same(a, b, where="result"):
    assert type(a) is type(b), where
    if isinstance(a, dict):
        assert a.keys() == b.keys(), where
        for k in a:
            _same(a[k], b[k], "%s[%r]" % (where, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "%s[%d]" % (where, i))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape, where
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), where
    elif isinstance(a, float):
        assert a == b or (a != a and b != b), where
    else:
        assert a == b, where


def test_two_handles_in_sequence():
    from mrcaudiocodec_amd import Handle
    runs = []
    for _ in range(2):
        h = Handle()
        try:
            runs.append(_run_all(h))
        finally:
            h.close()
            h.close()                                     # the second close does nothing
        assert h._h is None
    (first, ms), (second, _) = runs
    _same(second, first)
    assert len(first["chained", "stereo"]["bytes"]) > 0 and first["sensitivity"]["blocks_examined"] > 0
    for k, v in ms.items():
        assert np.all(np.isfinite(v)) and np.all(v >= 0), (k, v)


def test_two_live_handles():
    from mrcaudiocodec_amd import Handle
    a, b = Handle(target_bits_per_sample=2.0), Handle(target_bits_per_sample=4.0)
    try:
        run = lambda h: h.encode_chained_pac(STEREO[0:1], STEREO[1:2], [SHAPES], num_samples=[NS])["bytes"].tobytes()
        first_a, first_b = run(a), run(b)
        assert first_a != first_b                         # (two rates: two files)
        a.close()
        assert run(b) == first_b
    finally:
        a.close()
        b.close()


def test_kept_bytes_grow_between_time_slabs():
    """Slabs of two blocks (one per slab with the two rates' memory): the stream's packed bytes of both rungs are kept from
    slab to slab in a buffer that grows under them."""
    from mrcaudiocodec_amd import Handle
    run = lambda h: h.encode_chained_pac_target_nmr(STEREO[0:1], STEREO[1:2], [SHAPES], RATES, -3.0, num_samples=[NS])
    h = Handle()
    try:
        want = run(h)
    finally:
        h.close()
    h = Handle()
    try:
        h.set_option(OPT_SLAB_BLOCKS, 2)
        got = run(h)
    finally:
        h.close()
    assert _files(got) == _files(want) and len(want[0]["data"]) > 0
    _same(_measured(got), _measured(want))


def test_staging_buffers_reallocate_under_live_ones():
    from mrcaudiocodec_amd import Handle, synth
    fl, fr = synth.pcm_to_float(STEREO[0]), synth.pcm_to_float(STEREO[1])
    x = np.linspace(-1.0, 1.0, 4097)
    h = Handle()
    try:
        first = h.quantize_uniform(x, 8)                  # two staging buffers
        joint = h.encode_joint(_blocks(fl, 65), _blocks(fr, 65), HOP, HOP, want_mdct=True)   # more than any call before
        again = h.quantize_uniform(x, 8)
        _same(again, first)
        _same(h.encode_joint(_blocks(fl, 65), _blocks(fr, 65), HOP, HOP, want_mdct=True), joint)
    finally:
        h.close()
    assert len(np.unique(first)) > 2


def test_failed_create_leaves_the_next_handle_whole():
    from mrcaudiocodec_amd import Handle, MrcError, synth
    from oracle import fast
    with pytest.raises(MrcError):
        Handle(n_scale_bits=9)
    h = Handle()
    try:
        block = _blocks(synth.pcm_to_float(MONO[0]), 1)
        got = h.encode_mono(block, HOP, HOP)
    finally:
        h.close()
    ref = fast.encode_mono_batch(block, HOP, HOP)
    for k in ("overall_scale", "bit_alloc", "scale_factor", "mantissa", "reservoir_out"):
        assert np.array_equal(got[k], ref[k]), k
