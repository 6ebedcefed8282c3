"""
GPU tests of the constant-quality VBR encode to a file size (mrc_encode_vbr_size_pac, mrc_dev_encode_vbr_size_pac,
Handle.encode_vbr_size_pac, pacfile.encode_stream_vbr_size, cli --vbr-bytes).

The reference of every assertion is the EXISTING call, Handle.encode_vbr_nmr_pac, never the new one: per stream the file at
every ceiling of a small grid gives the table bytes(i); the targets are taken from that table when the test runs; the search
the new call reports must be pacfile.bisect_ceiling over the table, its file and numbers the existing call's at the chosen
ceiling.  Every comparison is equality.  The content is that of tests/test_gpu_vbr.py (the same generators and parameters).
"""
import ctypes as C
import json
import math

import numpy as np
import pytest

import chain_kit as kit
from chain_kit import HOP, handle as _handle

pytestmark = pytest.mark.gpu
LO, STEP, N = -12.0, 3.0, 8
SLAB_OPT, SLAB_DEFAULT = 6, 131072
NUMBERS = ("ceiling_ratio", "capped_bands", "coded_bits", "nmr_total_db", "nmr_max_db", "disturbed_blocks", "n_blocks")


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    kit.close_handles()
    _STREAMS.clear()


def _grid_db(i, lo=LO, step=STEP):
    return float(np.float64(lo) + np.float64(i) * np.float64(step))


class Stream:
    def __init__(self, pcm, rate=48000, exact=False, long_blocks=False, huffman=True):
        self.pcm, self.rate, self.huffman = pcm, rate, huffman
        self.h = _handle(exact, rate)
        self.mono = pcm.shape[0] == 1
        if long_blocks:
            self.shapes = np.array([(i * HOP, HOP, HOP) for i in range(pcm.shape[1] // HOP - 1)], np.int64)
        else:
            self.shapes = kit.shapes_to_last_long(self.h, pcm)
        self.ns = len(self.shapes) * HOP
        self._ref = {}

    def ref(self, db):
        """the EXISTING call at ceiling db: the reference"""
        if db not in self._ref:
            right = None if self.mono else self.pcm[1:2]
            self._ref[db] = self.h.encode_vbr_nmr_pac(self.pcm[0:1], right, [self.shapes], db, use_huffman=self.huffman,
                                                      num_samples=[self.ns])[0]
        return self._ref[db]

    def table(self, lo=LO, step=STEP, n=N):
        """bytes(i): the size of the existing call's file at every grid point"""
        return [len(self.ref(_grid_db(i, lo, step))["data"]) for i in range(n)]

    def size(self, target, lo=LO, step=STEP, n=N, **kw):
        """the call under test"""
        right = None if self.mono else self.pcm[1:2]
        return self.h.encode_vbr_size_pac(self.pcm[0:1], right, [self.shapes], [target], lo, step, n, use_huffman=self.huffman,
                                          num_samples=[self.ns], **kw)[0]


_STREAMS = {}


def _stream(name):
    if name not in _STREAMS:
        if name in ("stereo", "mono", "raw", "exact"):
            s = Stream(kit.clicks(12, 11, name == "mono", period=5), exact=name == "exact", huffman=name != "raw")
            assert len({(int(a), int(b)) for (_, a, b) in s.shapes}) == 4, "all four block shapes"
        elif name == "hi96":
            s = Stream(kit.noise(6, 3, 96000), rate=96000, long_blocks=True)
        else:                                            # "s<k>" stereo, "m<k>" mono: the many-stream calls, 4 .. 12 hops
            k = int(name[1:])
            s = Stream(kit.clicks(4 + 2 * k, 40 + 3 * k, name[0] == "m", period=5))
        _STREAMS[name] = s
    return _STREAMS[name]


def _targets(table):
    """the issue's four, from the table: bytes(k) for a middle k, one byte less, below the loosest, above the tightest"""
    k = len(table) // 2
    return dict(equal=table[k], one_below=table[k] - 1, not_met=table[-1] - 1, above_tightest=table[0] + 1)


def _check_against_table(s, got, target, table, lo=LO, step=STEP):
    """everything the call returned for one stream against the existing call and the rule over its table"""
    from mrcaudiocodec_amd import pacfile
    chosen, met, probed = pacfile.bisect_ceiling(table, target)
    print("target %d table %r -> chosen %d met %s probes %r; got chosen %d met %s probes %r bytes %r"
          % (target, table, chosen, met, probed, got["chosen"], got["met"], got["probe_index"], got["probe_bytes"]))
    assert got["chosen"] == chosen and got["met"] == met
    assert got["probes"] == len(probed) and got["probe_index"] == probed
    assert got["probe_bytes"] == [table[i] for i in probed]
    assert got["chosen_db"] == _grid_db(chosen, lo, step)
    want = s.ref(got["chosen_db"])
    assert got["data"] == want["data"]
    for k in NUMBERS:
        assert got[k] == want[k], (k, got[k], want[k])
    if met:
        assert len(got["data"]) <= target


@pytest.mark.parametrize("kind", ["equal", "one_below", "not_met", "above_tightest"])
@pytest.mark.parametrize("name", ["stereo", "mono", "raw", "exact", "hi96"])
def test_search_file_and_numbers_equal_the_existing_call(name, kind):
    s = _stream(name)
    table = s.table()
    assert len(set(table)) > 2, "the grid separates file sizes"
    target = _targets(table)[kind]
    got = s.size(target)
    _check_against_table(s, got, target, table)
    if kind == "not_met":
        assert not got["met"] and got["chosen"] == N - 1 and got["probes"] == 1
    if kind == "above_tightest":
        assert got["met"] and got["chosen"] == 0


def test_the_content_has_ms_bands_lr_bands_and_capped_bands():
    """what the walk's record must cover: a ceiling of the grid at which bands are capped, and a joint file"""
    s = _stream("stereo")
    tight = s.h.encode_vbr_size_pac(s.pcm[0:1], s.pcm[1:2], [s.shapes], [10 ** 9], -60.0, 3.0, 2, num_samples=[s.ns])[0]
    want = s.ref(-60.0)
    assert tight["chosen"] == 0 and tight["capped_bands"] == want["capped_bands"] > 0
    assert tight["data"] == want["data"]


def _many(prefix, count):
    """`count` streams of one kind, each with its table and a target of its own: stream i aims at bytes(1 + i mod (N - 2))"""
    sel = [_stream("%s%d" % (prefix, k)) for k in range(count)]
    tables = [s.table() for s in sel]
    targets = [t[1 + i % (N - 2)] for i, t in enumerate(tables)]
    return sel, tables, targets


@pytest.mark.parametrize("prefix,count", [("s", 5), ("m", 5)])
def test_streams_of_one_call_search_independently_whatever_the_slabs(prefix, count):
    sel, tables, targets = _many(prefix, count)
    h = sel[0].h
    assert len({len(s.shapes) for s in sel}) == count, "different lengths"
    left, right, _ = kit.rows([s.pcm for s in sel])
    shapes, ns = [s.shapes for s in sel], [s.ns for s in sel]
    many = h.encode_vbr_size_pac(left, right, shapes, targets, LO, STEP, N, num_samples=ns)
    for s, m, t, tab in zip(sel, many, targets, tables):
        _check_against_table(s, m, t, tab)
        single = s.size(t)
        for k in ("data", "chosen", "chosen_db", "met", "probes", "probe_index", "probe_bytes") + NUMBERS:
            assert m[k] == single[k], k
    assert len({m["chosen"] for m in many}) >= 2, "streams of one call end on different ceilings"
    # several whole-stream slabs: twice the longest stream's blocks leaves room for it and its record, not for all streams
    longest = max(len(sh) for sh in shapes)
    assert sum(len(sh) for sh in shapes) > 2 * longest
    try:
        h.set_option(SLAB_OPT, 2 * longest)
        slabbed = h.encode_vbr_size_pac(left, right, shapes, targets, LO, STEP, N, num_samples=ns)
    finally:
        h.set_option(SLAB_OPT, SLAB_DEFAULT)
    for m, m2 in zip(many, slabbed):
        assert m == m2


def test_device_entry_point():
    import torch
    sel, tables, targets = _many("s", 5)
    h = sel[0].h
    left, right, stride = kit.rows([s.pcm for s in sel])
    shapes, ns = [s.shapes for s in sel], [s.ns for s in sel]
    host = h.encode_vbr_size_pac(left, right, shapes, targets, LO, STEP, N, num_samples=ns)
    dev = torch.device("cuda", 0)
    dl, dr = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    total = sum(len(m["data"]) for m in host)
    out = torch.zeros(total + 64, dtype=torch.uint8, device=dev)
    got = h.encode_vbr_size_pac(None, None, shapes, targets, LO, STEP, N, num_samples=ns,
                                device=(dl.data_ptr(), dr.data_ptr(), stride, out.data_ptr(), total + 64))
    back = out.cpu().numpy()
    for g, m in zip(got, host):
        lo, hi = g["data"]
        g["data"] = back[lo:hi].tobytes()
        assert g == m
    assert not back[total:].any()


def test_one_ceiling():
    s = _stream("stereo")
    db = _grid_db(3)
    size = len(s.ref(db)["data"])
    for target, met in ((size, True), (size - 1, False), (size + 1000, True)):
        got = s.size(target, lo=db, step=1.0, n=1)
        _check_against_table(s, got, target, [size], lo=db, step=1.0)
        assert got["probes"] == 1 and got["met"] == met and got["chosen"] == 0 and got["chosen_db"] == db


def test_decodes_to_the_same_pcm():
    s = _stream("stereo")
    table = s.table()
    got = s.size(table[2])
    a = s.h.decode_pac_pcm16(got["data"], interleaved=False)[0]             # mrc_decode_pac_pcm16
    b = s.h.decode_pac_pcm16(s.ref(got["chosen_db"])["data"], interleaved=False)[0]
    assert a.shape == b.shape and a.shape[0] == 2 and np.array_equal(a, b)


def test_second_batch_of_one_shape_equals_the_existing_call_in_single_batch_slabs():
    """Inside a slab the blocks of one shape are recorded 16384 at a time.  One mono stream of (L,S), 16384 + 5 x (S,S), (S,L):
    the search keeps it in one slab (the default capacity, less the record, still holds its 16391 blocks), so its (S,S) group
    is a full batch and a batch of five; the existing call under 4096-block slabs runs single batches only."""
    pcm, shapes, ns = kit.long_short_run(period=5)
    db = -6.0
    h = _handle()
    try:
        h.set_option(SLAB_OPT, 4096)
        want = h.encode_vbr_nmr_pac(pcm, None, [shapes], db, num_samples=[ns])[0]
    finally:
        h.set_option(SLAB_OPT, SLAB_DEFAULT)
    target = len(want["data"])
    got = h.encode_vbr_size_pac(pcm, None, [shapes], [target], db, 1.0, 1, num_samples=[ns])[0]
    assert got["met"] and (got["chosen"], got["chosen_db"], got["probes"]) == (0, db, 1)
    assert got["probe_index"] == [0] and got["probe_bytes"] == [target]
    assert got["data"] == want["data"] and got["n_blocks"] == len(shapes) + 1
    for k in NUMBERS:
        assert got[k] == want[k], (k, got[k], want[k])


def _raw(s, target, lo=LO, step=STEP, n=N, out_cap=None, num_samples=True, off=None, a=None, b=None, no_target=False,
         trace=True):
    """the C entry point itself -> (rc, out, results)"""
    from mrcaudiocodec_amd import _lib
    h = s.h
    s0, o0, a0, b0 = h._chain_schedule([s.shapes])
    off = o0 if off is None else np.ascontiguousarray(off, np.int64)
    a = a0 if a is None else np.ascontiguousarray(a, np.int32)
    b = b0 if b is None else np.ascontiguousarray(b, np.int32)
    ns = np.ascontiguousarray([s.ns], np.uint32)
    tgt = np.ascontiguousarray([target], np.int64)
    cap = h.chain_out_bound(s0, a0, b0, True, True, 1 if s.mono else 2) if out_cap is None else out_cap
    out = np.full(max(cap, 1) + 32, 0xEE, np.uint8)
    left = np.ascontiguousarray(s.pcm[0:1])
    right = None if s.mono else np.ascontiguousarray(s.pcm[1:2])
    P = _lib.MRC_MAX_PROBES
    res = dict(s_off=np.zeros(2, np.int64), chosen=np.full(1, -7, np.int32), chosen_db=np.full(1, np.nan),
               ratio=np.full(1, np.nan), met=np.full(1, -7, np.int32), probes=np.full(1, -7, np.int32),
               p_idx=np.full(P, -7, np.int32), p_bytes=np.full(P, -7, np.int64), capped=np.full(1, -7, np.int64),
               bits=np.full(1, -7, np.int64), tot=np.full(1, np.nan), mx=np.full(1, np.nan), dist=np.full(1, -7, np.int64),
               nblk=np.full(1, -7, np.int64), total=np.full(1, -7, np.int64))
    p = lambda arr: arr.ctypes.data
    rc = _lib.lib.mrc_encode_vbr_size_pac(
        h._h, float(lo), float(step), int(n), None if no_target else p(tgt), 1, left.ctypes.data_as(C.c_void_p),
        None if s.mono else right.ctypes.data_as(C.c_void_p), left.shape[1], p(s0), p(off), p(a), p(b), 1,
        ns.ctypes.data_as(C.c_void_p) if num_samples else None, out.ctypes.data_as(C.c_void_p), cap, p(res["s_off"]),
        p(res["chosen"]), p(res["chosen_db"]), p(res["ratio"]), p(res["met"]), p(res["probes"]),
        p(res["p_idx"]) if trace else None, p(res["p_bytes"]) if trace else None, p(res["capped"]), p(res["bits"]),
        p(res["tot"]), p(res["mx"]), p(res["dist"]), p(res["nblk"]), p(res["total"]))
    return rc, out, res


def test_unused_trace_entries_are_minus_one_and_the_trace_is_optional():
    from mrcaudiocodec_amd import pacfile
    s = _stream("mono")
    table = s.table()
    target = table[N // 2]
    chosen, met, probed = pacfile.bisect_ceiling(table, target)
    rc, out, res = _raw(s, target)
    assert rc == 0 and int(res["probes"][0]) == len(probed)
    assert list(res["p_idx"]) == probed + [-1] * (9 - len(probed))
    assert list(res["p_bytes"]) == [table[i] for i in probed] + [-1] * (9 - len(probed))
    rc, out2, res2 = _raw(s, target, trace=False)
    assert rc == 0 and int(res2["chosen"][0]) == chosen == int(res["chosen"][0]) and np.array_equal(out, out2)
    assert np.all(res2["p_idx"] == -7) and np.all(res2["p_bytes"] == -7)


def test_refusals_name_the_argument():
    from mrcaudiocodec_amd import _lib
    s = _stream("stereo")
    h = s.h
    table = s.table()
    target = table[N // 2]
    _, off, a, b = h._chain_schedule([s.shapes])

    def refused(word, **kw):
        rc, out, res = _raw(s, kw.pop("target", target), **kw)
        msg = _lib.lib.mrc_last_error(h._h).decode()
        assert rc == _lib.MRC_ERR_INVALID and word in msg, (rc, msg)
        assert np.all(out == 0xEE) and int(res["total"][0]) == -7, "refused before any work"

    # what mrc_encode_vbr_nmr_pac refuses
    refused("num_samples", num_samples=False)
    h.set_option(5, 1)
    try:
        refused("MRC_OPT_SENSITIVITY")
    finally:
        h.set_option(5, 0)
    first_short = a.copy()
    first_short[0] = 128
    refused("first block", a=first_short)
    shifted = off.copy()
    shifted[3] += 64
    refused("block_offset[3]", off=shifted)
    ends_short = b.copy()
    ends_short[-1] = 128
    refused("last block", b=ends_short)
    # its own
    for bad in (math.nan, math.inf, -math.inf):
        refused("ceiling_lo_db", lo=bad)
        refused("ceiling_step_db", step=bad)
    refused("ceiling_step_db", step=0.0)
    refused("ceiling_step_db", step=-3.0)
    for bad in (0, -1, 257):
        refused("n_ceilings", n=bad)
    refused("target_bytes", no_target=True)
    refused("target_bytes[0]", target=-1)
    # a stream that would run in time slabs
    try:
        h.set_option(SLAB_OPT, 4)
        assert len(s.shapes) > 4
        refused("MRC_OPT_CHAIN_SLAB_BLOCKS")
        refused("stream 0")
    finally:
        h.set_option(SLAB_OPT, SLAB_DEFAULT)
    got = s.size(target)                                 # the handle still works
    _check_against_table(s, got, target, table)


def test_out_cap_too_small():
    from mrcaudiocodec_amd import _lib, pacfile
    s = _stream("stereo")
    h = s.h
    table = s.table()
    target = table[N // 2]
    chosen, met, probed = pacfile.bisect_ceiling(table, target)
    want = s.ref(_grid_db(chosen))
    size = len(want["data"])
    rc, out, res = _raw(s, target, out_cap=size - 1)
    assert rc == _lib.MRC_ERR_NOMEM
    assert int(res["total"][0]) == size and list(res["s_off"]) == [0, size]
    assert (int(res["chosen"][0]), int(res["met"][0]), int(res["probes"][0])) == (chosen, int(met), len(probed))
    assert res["chosen_db"][0] == _grid_db(chosen) and res["ratio"][0] == want["ceiling_ratio"]
    assert list(res["p_idx"][:len(probed)]) == probed and list(res["p_bytes"][:len(probed)]) == [table[i] for i in probed]
    assert res["tot"][0] == want["nmr_total_db"] and res["mx"][0] == want["nmr_max_db"]
    assert (int(res["capped"][0]), int(res["bits"][0]), int(res["dist"][0]), int(res["nblk"][0])) == (
        want["capped_bands"], want["coded_bits"], want["disturbed_blocks"], want["n_blocks"])
    assert np.all(out[size - 1:] == 0xEE), "nothing is written past out_cap"
    buf = np.zeros(size, np.uint8)
    total = np.zeros(1, np.int64)
    assert _lib.lib.mrc_chain_fetch_output(h._h, buf.ctypes.data_as(C.c_void_p), buf.size, total.ctypes.data) == 0
    assert buf.tobytes() == want["data"] and int(total[0]) == size
    assert s.size(target, out_cap=16)["data"] == want["data"]           # the binding does the same on its own
    rc, out, res = _raw(s, target, out_cap=size)
    assert rc == 0 and out[:size].tobytes() == want["data"] and np.all(out[size:] == 0xEE)


def test_cli_vbr_bytes(tmp_path, capsys):
    from mrcaudiocodec_amd import cli, pacfile
    s = _stream("stereo")
    # the WAV: the stream without its prior hop, up to the end of its last block, and one more (silent) hop that is never coded
    pcm = np.concatenate([s.pcm[:, HOP:HOP + s.ns], np.zeros((2, HOP), np.int16)], axis=1)
    wav, dst = str(tmp_path / "in.wav"), str(tmp_path / "out.pac")
    kit.write_wav(wav, pcm)
    h = s.h
    codes = np.concatenate([np.zeros((2, HOP), np.int16), pcm], axis=1)
    from mrcaudiocodec_amd import transient
    shapes = transient.block_shape_array(h, codes)
    ns = pcm.shape[1]
    sizes = [len(pacfile.encode_stream_vbr_nmr(h, codes, shapes, _grid_db(i), num_samples=ns)["data"]) for i in range(N)]
    target = sizes[3]
    capsys.readouterr()
    cli.main([wav, dst, "--vbr-bytes", str(target), "--vbr-grid", "%g:%g:%d" % (LO, STEP, N)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    data = open(dst, "rb").read()
    lib = pacfile.encode_stream_vbr_size(h, codes, shapes, target, LO, STEP, N, num_samples=ns)
    chosen, met, probed = pacfile.bisect_ceiling(sizes, target)
    assert data == lib["data"] and line["bytes"] == len(data) <= target
    assert (lib["chosen"], lib["met"], lib["probe_index"]) == (chosen, met, probed)
    assert data == pacfile.encode_stream_vbr_nmr(h, codes, shapes, _grid_db(chosen), num_samples=ns)["data"]
    assert line["chosen_db"] == lib["chosen_db"] == _grid_db(chosen) and line["met"] is True and line["probes"] == len(probed)
    for k in ("coded_bits", "capped_bands", "nmr_total_db", "nmr_max_db", "disturbed_blocks", "n_blocks", "ceiling_ratio"):
        assert line[k] == lib[k], k
    # --vbr-bits-per-sample: the same search at the size the stated formula gives
    coded = int(sum(int(b) for (_, _, b) in shapes))
    bps = 8.0 * (target - len(pacfile.header(h.cfg, 2, ns)) - 4 * 2 * (len(shapes) + 1)) / (coded * 2)
    want_bytes = cli.vbr_size_target_bytes(bps, len(pacfile.header(h.cfg, 2, ns)), coded, 2, 2 * (len(shapes) + 1))
    cli.main([wav, dst, "--vbr-bits-per-sample", repr(bps), "--vbr-grid", "%g:%g:%d" % (LO, STEP, N)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["target_bytes"] == want_bytes
    c2, m2, _ = pacfile.bisect_ceiling(sizes, want_bytes)
    assert line["chosen_db"] == _grid_db(c2) and line["met"] == m2
    assert open(dst, "rb").read() == pacfile.encode_stream_vbr_nmr(h, codes, shapes, _grid_db(c2), num_samples=ns)["data"]
