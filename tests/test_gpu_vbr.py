"""
GPU tests of the constant-quality VBR encode (mrc_encode_vbr_nmr_pac, Handle.encode_vbr_nmr_pac,
pacfile.encode_stream_vbr_nmr, cli --vbr-nmr) against the NumPy restatement of its rule (tests/vbr_restatement.py), the
existing measure (mrc_pac_nmr) and the existing decoders.

The seeds were chosen on the CPU so that the restatement meets no EDGE candidate (a ratio within 1e-6 of the ceiling, two
error energies within 1e-6 of each other) on any stream and ceiling used here; each test asserts that this is still so.
With it every comparison is equality: the same bytes, the same doubles, the same counts.
"""
import ctypes as C
import json
import math

import numpy as np
import pytest

import chain_kit as kit
import nmr_restatement as nr
import vbr_restatement as vr
from chain_kit import HOP, handle as _handle, handles_closed_after_module as _close_handles  # noqa: F401

pytestmark = pytest.mark.gpu
CEILINGS = (6.0, 0.0, -6.0, -60.0)


class Stream:
    def __init__(self, pcm, rate=48000, exact=False, long_blocks=False):
        self.pcm, self.rate, self.exact = pcm, rate, exact
        self.h = _handle(exact, rate)
        self.mono = pcm.shape[0] == 1
        if long_blocks:
            self.shapes = np.array([(i * HOP, HOP, HOP) for i in range(pcm.shape[1] // HOP - 1)], np.int64)
        else:
            self.shapes = kit.shapes_to_last_long(self.h, pcm)
        self.ns = len(self.shapes) * HOP
        self.src = vr.source_of(pcm, self.shapes, HOP)
        self._got, self._want = {}, {}

    def run(self, db, **kw):
        right = None if self.mono else self.pcm[1:2]
        return self.h.encode_vbr_nmr_pac(self.pcm[0:1], right, [self.shapes], db, num_samples=[self.ns], **kw)[0]

    def got(self, db):
        if db not in self._got:
            self._got[db] = self.run(db)
        return self._got[db]

    def want(self, db, c):
        if db not in self._want:
            self._want[db] = vr.encode(self.pcm, self.shapes, c, sample_rate=self.rate, num_samples=self.ns)
        return self._want[db]


_STREAMS = {}


def _stream(name):
    if name not in _STREAMS:
        if name == "stereo":
            s = Stream(kit.clicks(12, 11, False, period=5))
            assert len({(int(a), int(b)) for (_, a, b) in s.shapes}) == 4, "all four block shapes"
        elif name == "mono":
            s = Stream(kit.clicks(12, 11, True, period=5))
            assert len({(int(a), int(b)) for (_, a, b) in s.shapes}) == 4, "all four block shapes"
        elif name == "hi96":
            s = Stream(kit.noise(6, 3, 96000), rate=96000, long_blocks=True)
        elif name == "exact":
            s = Stream(kit.clicks(12, 11, False, period=5), exact=True)
        else:                                            # "s<k>": the streams of the 5-stream call, 4 .. 12 hops
            k = int(name[1:])
            s = Stream(kit.clicks(4 + 2 * k, 40 + 3 * k, bool(k & 1), period=5))
        _STREAMS[name] = s
    return _STREAMS[name]


def _first_difference(s, got, want):
    """the first (block, stream, band) whose bits differ, with the restatement's r there"""
    _, nch, blocks = nr.parse_file(got["data"])
    k = 0
    for i, (a, b, joint, p, _) in enumerate(blocks):
        parts = [p] if joint else p
        for q in parts:
            info = want["blocks"][k]
            k += 1
            bas = q["bitAlloc"] if joint else [q["bitAlloc"]]
            for strm, ba in enumerate(bas):
                for j, (g, w) in enumerate(zip(ba, info["ba"][strm])):
                    if int(g) != int(w):
                        return "block %d (%d,%d) stream %d band %d: %d bits, restatement %d with r = %r, trail %r" % (
                            i, a, b, strm, j, g, w, info["r"][strm][j], info["trail"][strm][j] or info["trail"][0][j])
    return "same allocations: scale factors, mantissas, tables or framing differ"


def _check(s, db):
    g = s.got(db)
    assert g["ceiling_ratio"] == vr.ceiling_ratio(db), (g["ceiling_ratio"], vr.ceiling_ratio(db))
    w = s.want(db, g["ceiling_ratio"])
    assert w["edges"] == 0, "the input was chosen to have no edge candidate"
    if g["data"] != w["data"]:
        pytest.fail("ceiling %g dB: %d bytes, restatement %d; %s" % (db, len(g["data"]), len(w["data"]), _first_difference(s, g, w)))
    assert g["capped_bands"] == w["capped"] and g["coded_bits"] == vr.coded_bits(w["data"], w["nch"])
    return g, w


@pytest.mark.parametrize("db", CEILINGS)
@pytest.mark.parametrize("name", ["stereo", "mono"])
def test_bytes_equal_the_restatement(name, db):
    s = _stream(name)
    g, w = _check(s, db)
    if name == "stereo" and db == 0.0:
        ms = [blk["ms"] for blk in w["blocks"] if blk["ms"] is not None]
        assert any((m == 1).any() for m in ms) and any((m != 1).any() for m in ms), "M/S and L/R bands"
    if db == -60.0:
        assert g["capped_bands"] > 0, "the cap is reached"


def test_bytes_at_96_khz_where_masks_are_infinite():
    s = _stream("hi96")
    g, w = _check(s, 0.0)
    m = nr.restate(g["data"], s.src)
    assert any(np.isinf(e["mask"]).any() for e in m["entries"]), "bands whose mask is +inf"


@pytest.mark.parametrize("db", CEILINGS)
@pytest.mark.parametrize("name", ["stereo", "mono", "hi96"])
def test_numbers_are_the_measure_of_the_file(name, db):
    from mrcaudiocodec_amd import pacfile
    s = _stream(name)
    g = s.got(db)
    m = pacfile.measure_nmr(s.h, [g["data"]], [s.src])[0]
    for k in ("nmr_total_db", "nmr_max_db", "disturbed_blocks", "n_blocks"):
        assert g[k] == m[k], (k, g[k], m[k])
    assert g["n_blocks"] == len(s.shapes) + 1
    if g["capped_bands"] == 0:
        # the slack is for the host's log10 alone: max r <= c holds exactly on the device
        assert g["nmr_max_db"] <= 10.0 * math.log10(g["ceiling_ratio"]) + 1e-9
        if db == 0.0:
            assert g["disturbed_blocks"] == 0


@pytest.mark.parametrize("name", ["stereo", "mono"])
def test_decodes_like_the_oracle(name):
    from oracle import decode as odec
    s = _stream(name)
    g = s.got(-6.0)
    pcm = s.h.decode_pac_pcm16(g["data"], interleaved=False)[0]        # mrc_decode_pac_pcm16
    _, want = odec.decode_pac(g["data"])
    want = odec.pcm16(np.atleast_2d(want)[:, HOP:])
    assert pcm.shape == want.shape and np.array_equal(pcm, want)


def test_infinite_ceilings():
    s = _stream("stereo")
    g = s.run(math.inf)
    assert g["ceiling_ratio"] == math.inf and g["capped_bands"] == 0
    _, _, blocks = nr.parse_file(g["data"])
    for (_, _, joint, p, _) in blocks:
        for q in ([p] if joint else p):
            assert not np.any(np.concatenate([np.ravel(x) for x in (q["bitAlloc"] if joint else [q["bitAlloc"]])]))
    g = s.run(-math.inf)                                 # c = 0: met only where the noise is exactly 0
    assert g["ceiling_ratio"] == 0.0 and g["capped_bands"] > 0


def _same(a, b):
    for k in ("data", "capped_bands", "coded_bits", "nmr_total_db", "nmr_max_db", "disturbed_blocks", "n_blocks", "ceiling_ratio"):
        assert a[k] == b[k], k


def test_independent_of_slabs_batching_and_entry_point():
    import torch
    names = ["s%d" % k for k in range(5)]
    streams = [_stream(n) for n in names]
    h = _handle()
    db = -6.0
    singles = [s.got(db) for s in streams]
    for s in streams:
        _check(s, db)
    assert len({len(s.shapes) for s in streams}) == 5, "different lengths"
    # one call of the three stereo streams, one of the two mono streams, rows padded to one stride
    for mono in (False, True):
        sel = [s for s in streams if s.mono == mono]
        left, right, stride = kit.rows([s.pcm for s in sel])
        shapes, ns = [s.shapes for s in sel], [s.ns for s in sel]
        many = h.encode_vbr_nmr_pac(left, right, shapes, db, num_samples=ns)
        for s, m in zip(sel, many):
            _same(m, s.got(db))
        for m, m2 in zip(many, h.encode_vbr_nmr_pac(left, right, shapes, db, num_samples=ns)):
            _same(m, m2)                                 # a repeated call
        try:
            h.set_option(6, 1)                           # the smallest slab: every stream in time slabs of one block
            for s, m in zip(sel, h.encode_vbr_nmr_pac(left, right, shapes, db, num_samples=ns)):
                _same(m, s.got(db))
            h.set_option(6, max(len(sh) for sh in shapes))   # whole streams, several slabs
            for s, m in zip(sel, h.encode_vbr_nmr_pac(left, right, shapes, db, num_samples=ns)):
                _same(m, s.got(db))
        finally:
            h.set_option(6, 131072)
        # device memory in and out
        dev = torch.device("cuda", 0)
        dl = torch.from_numpy(left).to(dev)
        dr = None if mono else torch.from_numpy(right).to(dev)
        total = sum(len(m["data"]) for m in many)
        out = torch.zeros(total + 64, dtype=torch.uint8, device=dev)
        got = h.encode_vbr_nmr_pac(None, None, shapes, db, num_samples=ns,
                                   device=(dl.data_ptr(), None if mono else dr.data_ptr(), stride, out.data_ptr(), total + 64))
        host = out.cpu().numpy()
        for g, m in zip(got, many):
            lo, hi = g["data"]
            g["data"] = host[lo:hi].tobytes()
            _same(g, m)
        assert not host[total:].any()


def test_second_batch_of_one_shape_equals_single_batch_slabs():
    """Inside a slab the blocks of one shape are analysed 16384 at a time.  4096-block slabs: time slabs of one batch each,
    the path of every other test; the default slab: one slab whose (S,S) group is a full batch and a batch of five."""
    h = _handle()
    pcm, shapes, ns = kit.long_short_run(period=5)
    run = lambda: h.encode_vbr_nmr_pac(pcm, None, [shapes], -6.0, num_samples=[ns])[0]
    try:
        h.set_option(6, 4096)
        want = run()
        h.set_option(6, 131072)
        got = run()
    finally:
        h.set_option(6, 131072)
    assert want["n_blocks"] == len(shapes) + 1 and len(want["data"]) > 0
    _same(got, want)


def test_exact_spreading_mode():
    from mrcaudiocodec_amd import pacfile
    s = _stream("exact")
    g = s.got(0.0)
    m = pacfile.measure_nmr(s.h, [g["data"]], [s.src])[0]          # (the same handle: exact spreading on both sides)
    for k in ("nmr_total_db", "nmr_max_db", "disturbed_blocks", "n_blocks"):
        assert g[k] == m[k], (k, g[k], m[k])
    assert g["capped_bands"] == 0 and g["disturbed_blocks"] == 0
    assert g["nmr_max_db"] <= 1e-9


def _raw(s, db, out_cap=None, num_samples=True, off=None, a=None, b=None):
    """the C entry point itself -> (rc, out, results)"""
    from mrcaudiocodec_amd import _lib
    h = s.h
    s0, o0, a0, b0 = h._chain_schedule([s.shapes])
    off = o0 if off is None else np.ascontiguousarray(off, np.int64)
    a = a0 if a is None else np.ascontiguousarray(a, np.int32)
    b = b0 if b is None else np.ascontiguousarray(b, np.int32)
    ns = np.ascontiguousarray([s.ns], np.uint32)
    cap = h.chain_out_bound(s0, a0, b0, True, True, 1 if s.mono else 2) if out_cap is None else out_cap
    out = np.full(max(cap, 1) + 32, 0xEE, np.uint8)
    left = np.ascontiguousarray(s.pcm[0:1])
    right = None if s.mono else np.ascontiguousarray(s.pcm[1:2])
    res = dict(s_off=np.zeros(2, np.int64), ratio=np.full(1, np.nan), capped=np.full(1, -7, np.int64),
               bits=np.full(1, -7, np.int64), tot=np.full(1, np.nan), mx=np.full(1, np.nan), dist=np.full(1, -7, np.int64),
               nblk=np.full(1, -7, np.int64), total=np.full(1, -7, np.int64))
    p = lambda arr: arr.ctypes.data
    rc = _lib.lib.mrc_encode_vbr_nmr_pac(
        h._h, float(db), 1, left.ctypes.data_as(C.c_void_p), None if s.mono else right.ctypes.data_as(C.c_void_p),
        left.shape[1], p(s0), p(off), p(a), p(b), 1, ns.ctypes.data_as(C.c_void_p) if num_samples else None,
        out.ctypes.data_as(C.c_void_p), cap, p(res["s_off"]), p(res["ratio"]), p(res["capped"]), p(res["bits"]), p(res["tot"]),
        p(res["mx"]), p(res["dist"]), p(res["nblk"]), p(res["total"]))
    return rc, out, res


def test_refusals_name_the_argument():
    from mrcaudiocodec_amd import _lib
    s = _stream("stereo")
    h = s.h
    _, off, a, b = h._chain_schedule([s.shapes])

    def refused(word, db=0.0, **kw):
        rc, out, _ = _raw(s, db, **kw)
        msg = _lib.lib.mrc_last_error(h._h).decode()
        assert rc == _lib.MRC_ERR_INVALID and word in msg, (rc, msg)
        assert np.all(out == 0xEE)

    refused("ceiling_db", db=math.nan)
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
    _same(s.run(0.0), s.got(0.0))                        # the handle still works


def test_out_cap_too_small():
    from mrcaudiocodec_amd import _lib
    s = _stream("stereo")
    h = s.h
    want = s.got(0.0)
    rc, out, res = _raw(s, 0.0, out_cap=len(want["data"]) - 1)
    assert rc == _lib.MRC_ERR_NOMEM
    assert int(res["total"][0]) == len(want["data"]) and list(res["s_off"]) == [0, len(want["data"])]
    assert res["tot"][0] == want["nmr_total_db"] and res["mx"][0] == want["nmr_max_db"]
    assert (int(res["capped"][0]), int(res["bits"][0]), int(res["dist"][0]), int(res["nblk"][0])) == (
        want["capped_bands"], want["coded_bits"], want["disturbed_blocks"], want["n_blocks"])
    assert np.all(out[len(want["data"]) - 1:] == 0xEE), "nothing is written past out_cap"
    buf = np.zeros(len(want["data"]), np.uint8)
    total = np.zeros(1, np.int64)
    assert _lib.lib.mrc_chain_fetch_output(h._h, buf.ctypes.data_as(C.c_void_p), buf.size, total.ctypes.data) == 0
    assert buf.tobytes() == want["data"] and int(total[0]) == len(want["data"])
    assert s.run(0.0, out_cap=16)["data"] == want["data"]           # the binding does the same on its own
    rc, out, res = _raw(s, 0.0, out_cap=len(want["data"]))
    assert rc == 0 and out[:len(want["data"])].tobytes() == want["data"] and np.all(out[len(want["data"]):] == 0xEE)


def test_cli_vbr_nmr(tmp_path, capsys):
    from mrcaudiocodec_amd import cli
    s = _stream("stereo")
    # the WAV: the stream without its prior hop, up to the end of its last block, and one more hop the encoder never codes
    pcm = np.concatenate([s.src, np.zeros((2, HOP), np.int16)], axis=1)
    wav, dst, back = str(tmp_path / "in.wav"), str(tmp_path / "out.pac"), str(tmp_path / "back.wav")
    kit.write_wav(wav, pcm)
    capsys.readouterr()
    cli.main([wav, dst, "--vbr-nmr", "0"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    r = cli.encode_wav_vbr_nmr(wav, None, "0")
    data = open(dst, "rb").read()
    assert data == r["data"] and line["bytes"] == len(data)
    for k in ("coded_bits", "capped_bands", "nmr_total_db", "nmr_max_db", "disturbed_blocks", "n_blocks", "bits_per_sample",
              "ceiling_ratio"):
        assert line[k] == r[k], k
    assert line["capped_bands"] == 0 and line["disturbed_blocks"] == 0 and line["nmr_max_db"] <= 1e-9
    cli.main([dst, back, "-d"])
    out = capsys.readouterr().out
    n_ch, n = (int(v) for v in out.split(":")[1].replace("channels x", "").replace("samples", "").split())
    from oracle import decode as odec
    assert n_ch == 2 and n == np.atleast_2d(odec.decode_pac(data)[1]).shape[1] - HOP
    for extra in (["-d"], ["--certify"], ["--measure"], ["--bits-per-sample", "4"], ["--target-nmr", "0"]):
        with pytest.raises(SystemExit):
            cli.main([wav, dst, "--vbr-nmr", "0"] + extra)
    with pytest.raises(SystemExit):
        cli.main([wav, dst, "--vbr-nmr", "nan"])
    capsys.readouterr()
