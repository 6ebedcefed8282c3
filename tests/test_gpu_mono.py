"""
Mono `.pac` files through the chained encode (pcm_right == NULL): the CLI against the reference's own mono bytes
(tests/golden/ref_pac_mono.npz), the round trip through every decoder, many streams in one call against the stream
encoded alone / block by block / by the oracle, the resident form, slabs, the output bound, the reservoir handover,
the sensitivity count, refusals, and stereo through the same entry points unchanged.
"""
import ctypes as C
import os

import numpy as np
import pytest

import chain_kit as kit
import mono_oracle as MO
from chain_kit import handles_closed_after_module as _close_handles  # noqa: F401

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_pac_mono.npz")
L = 1024
OPT_SLAB = 6                                          # MRC_OPT_CHAIN_SLAB_BLOCKS


def _fixture():
    if not os.path.exists(FIXTURE):
        pytest.skip("tests/golden/ref_pac_mono.npz not generated")
    return np.load(FIXTURE)


def _cases():
    return [str(c) for c in np.load(FIXTURE)["cases"]] if os.path.exists(FIXTURE) else ["missing"]


def _handle(rate=48000):
    return kit.handle(rate=rate)


def _write_wav(tmp_path, pcm, rate, name="in.wav"):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(MO.wav_bytes(pcm, rate))
    return p


def _streams(n, seed=1234):
    """n mono int16 streams of mixed length and content, each with the zero prior hop in front and two silent hops at
    the end (so that the detector's last written block is long, as Close() needs) -> (codes [n][stride], shapes,
    num_samples)."""
    from mrcaudiocodec_amd import transient
    h = _handle()
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 12, n) * L + rng.integers(0, L, n)
    stride = int((-(-lens.max() // L) + 3) * L)
    codes = np.zeros((n, stride), np.int16)
    shapes, num = [], []
    for s in range(n):
        m = int(lens[s])
        kind = s % 4
        t = np.arange(m)
        if kind == 0:
            x = rng.normal(0, 0.1 * 32767, m) * 10.0 ** (-2.0 * ((t // L) % 3 == 1))
        elif kind == 1:
            x = rng.uniform(2000, 12000) * np.sin(2 * np.pi * rng.uniform(100, 4000) / 48000 * t)
        elif kind == 2:
            x = rng.normal(0, 3.0, m)
        else:
            x = rng.normal(0, 0.02 * 32767, m)
            for p in rng.integers(0, max(m - 128, 1), 2):
                x[p:p + 128] = rng.normal(0, 0.5 * 32767, len(x[p:p + 128]))
        codes[s, L:L + m] = np.clip(np.rint(x), -32767, 32767).astype(np.int16)
        n_hops = -(-m // L) + 2
        sh = transient.block_shape_array(h, codes[s:s + 1, :(n_hops + 1) * L])
        assert sh[-1, 2] == L
        shapes.append(sh)
        num.append(m)
    return codes, shapes, num


@pytest.fixture(scope="module")
def many():
    codes, shapes, num = _streams(600)
    h = _handle()
    r = h.encode_chained_pac(codes, None, shapes, num_samples=num, want_trace=True, want_items=True)
    return codes, shapes, num, r


def _files(r, n):
    d, o = r["bytes"], r["stream_offset"]
    return [d[o[s]:o[s + 1]].tobytes() for s in range(n)]


# ---------------------------------------------------------------- the CLI against the reference's own mono files
@pytest.mark.parametrize("exact_spread", [False, True])
@pytest.mark.parametrize("huffman", [True, False])
@pytest.mark.parametrize("case", _cases())
def test_cli_mono_bytes_equal_reference(tmp_path, case, huffman, exact_spread):
    from mrcaudiocodec_amd import cli
    g = _fixture()
    pcm, rate = g[case + "_pcm"], int(g[case + "_rate"])
    wav = _write_wav(tmp_path, pcm, rate)
    got = cli.encode_wav(wav, str(tmp_path / "out.pac"), use_huffman=huffman, exact_spread=exact_spread)
    assert got == g[case + ("_pac" if huffman else "_pac_raw")].tobytes()
    assert open(str(tmp_path / "out.pac"), "rb").read() == got


@pytest.mark.parametrize("case", _cases())
def test_mono_round_trip_every_decoder(tmp_path, case):
    from mrcaudiocodec_amd import cli, pacfile
    from oracle import decode as odec
    g = _fixture()
    pcm, rate = g[case + "_pcm"], int(g[case + "_rate"])
    pac = g[case + "_pac"].tobytes()
    want = odec.pcm16(odec.decode_pac(pac)[1])[:, L:]
    assert want.shape[0] == 1
    p = str(tmp_path / "x.pac")
    with open(p, "wb") as f:
        f.write(pac)
    got_cli = cli.decode_pac_file(p, str(tmp_path / "x.wav"))
    assert np.array_equal(got_cli, want)
    h = _handle(rate)
    assert np.array_equal(pacfile.decode_pac_pcm16(h, pac), want)
    assert np.array_equal(h.decode_pac_pcm16(pac, interleaved=False)[0], want)


# ---------------------------------------------------------------- many streams in one call
def test_many_mono_streams_each_equal_alone_and_per_block(many):
    from mrcaudiocodec_amd import pacfile
    codes, shapes, num, r = many
    h = _handle()
    files = _files(r, len(shapes))
    for s in range(len(shapes)):
        alone = pacfile.encode_mono_stream(h, codes[s], shapes[s], num_samples=num[s])
        assert files[s] == alone, "stream %d" % s
        assert files[s][:4] == b"PAC " and int.from_bytes(files[s][8:10], "little") == 1
    for s in range(0, len(shapes), 7):
        per = pacfile.encode_mono_stream_per_block(h, MO.to_float(codes[s]), [tuple(x) for x in shapes[s].tolist()],
                                                   num_samples=num[s])
        assert files[s] == per, "stream %d" % s


def test_many_mono_streams_against_oracle_and_trace(many):
    from oracle import codec
    codes, shapes, num, r = many
    files = _files(r, len(shapes))
    base = np.concatenate([[0], np.cumsum([len(sh) + 1 for sh in shapes])])
    for s in list(range(8)) + [301, 599]:
        cp = codec.default_params(nChannels=1)
        trace = []
        want = MO.encode_mono_stream(MO.to_float(codes[s])[None], [tuple(x) for x in shapes[s].tolist()], cp, True,
                                     num_samples=num[s], trace=trace)
        assert files[s] == want, "stream %d" % s
        assert r["reservoir_trace"][base[s]:base[s + 1]].tolist() == trace, "stream %d" % s
        assert int(r["reservoir_out"][s]) == trace[-1]


def test_many_mono_streams_item_offsets(many):
    from mrcaudiocodec_amd import pacfile
    codes, shapes, num, r = many
    so, io = r["stream_offset"], r["item_offset"]
    assert len(io) == sum(len(sh) + 1 for sh in shapes) + 1 and io[-1] == r["total"]
    files = _files(r, len(shapes))
    k = 0
    for s in range(len(shapes)):
        _, nch, _, hl = pacfile.read_header(files[s])
        assert nch == 1
        chunks = pacfile.scan_chunks(files[s], hl)
        assert len(chunks) == len(shapes[s]) + 1
        assert np.array_equal(io[k:k + len(chunks)] - so[s], chunks), "stream %d" % s
        k += len(chunks)


# ---------------------------------------------------------------- resident form
@pytest.mark.parametrize("fmt", ["int16", "float64"])
def test_mono_resident_equals_host(fmt):
    import torch
    from mrcaudiocodec_amd.batch import StreamEncoder
    codes, shapes, num = _streams(40, seed=77)
    h = _handle()
    x = codes if fmt == "int16" else MO.to_float(codes)
    want = h.encode_chained_pac(x, None, shapes, num_samples=num, want_items=True, want_trace=False)
    enc = StreamEncoder(handle=h)
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    got = enc.encode_chained_pac(t, None, shapes, num_samples=num, want_items=True)
    assert got["bytes"].cpu().numpy().tobytes() == want["bytes"].tobytes()
    assert np.array_equal(got["stream_offset"], want["stream_offset"])
    assert np.array_equal(got["item_offset"], want["item_offset"])
    assert np.array_equal(got["reservoir_out"], want["reservoir_out"])
    if fmt == "float64":
        w16 = h.encode_chained_pac(codes, None, shapes, num_samples=num)
        assert w16["bytes"].tobytes() == want["bytes"].tobytes()


# ---------------------------------------------------------------- slabs
@pytest.mark.parametrize("which", ["time", "whole"])
def test_mono_slabs_equal_unslabbed(which):
    h = _handle()
    if which == "time":
        rng = np.random.default_rng(5)
        from mrcaudiocodec_amd import transient
        n = 300 * L
        x = rng.normal(0, 0.05 * 32767, n)
        for p in rng.integers(0, n - 128, 20):
            x[p:p + 128] = rng.normal(0, 0.6 * 32767, 128)
        codes = np.zeros((1, n + 3 * L), np.int16)
        codes[0, L:L + n] = np.clip(np.rint(x), -32767, 32767)
        shapes = [transient.block_shape_array(h, codes)]
        assert shapes[0][-1, 2] == L
        num, slab = [n], 64
    else:
        codes, shapes, num = _streams(50, seed=9)
        slab = 40
    kw = dict(num_samples=num, want_trace=True, want_items=True)
    was = h.get_option(OPT_SLAB)
    want = h.encode_chained_pac(codes, None, shapes, **kw)
    try:
        h.set_option(OPT_SLAB, slab)
        got = h.encode_chained_pac(codes, None, shapes, **kw)
    finally:
        h.set_option(OPT_SLAB, was)
    assert got["bytes"].tobytes() == want["bytes"].tobytes()
    for k in ("stream_offset", "item_offset", "reservoir_out", "reservoir_trace"):
        assert np.array_equal(got[k], want[k]), k


# ---------------------------------------------------------------- output bound, short buffer, fetch
def test_mono_short_buffer_nomem_then_fetch_and_bound():
    from mrcaudiocodec_amd import _lib
    codes, shapes, num = _streams(30, seed=31)
    h = _handle()
    want = h.encode_chained_pac(codes, None, shapes, num_samples=num)
    start, off, a, b = h._chain_schedule(shapes)
    bound = h.chain_out_bound(start, a, b, True, True, n_channels=1)
    assert bound >= want["total"] and bound > 0
    assert h.chain_out_bound(start, a, b, True, True, n_channels=2) > bound
    for s in range(len(shapes)):
        one = h.chain_out_bound(np.array([0, len(shapes[s])]), shapes[s][:, 1], shapes[s][:, 2], True, True, 1)
        assert one >= want["stream_offset"][s + 1] - want["stream_offset"][s]
    pl = np.ascontiguousarray(codes)
    n = len(shapes)
    ns = np.ascontiguousarray(num, dtype=np.uint32)
    so = np.zeros(n + 1, np.int64)
    total = np.zeros(1, np.int64)
    buf = np.zeros(want["total"] // 3, np.uint8)
    vp = lambda arr: arr.ctypes.data_as(C.c_void_p)
    P = lambda arr, t: arr.ctypes.data_as(t)
    rc = _lib.lib.mrc_encode_chained_stream_pac(h._h, n, vp(pl), None, 1, pl.shape[1], P(start, _lib._i64p),
                                                P(off, _lib._i64p), P(a, _lib._i32p), P(b, _lib._i32p), None, 1, 1, vp(ns),
                                                vp(buf), buf.size, P(so, _lib._i64p), None, None, None, P(total, _lib._i64p))
    assert rc == _lib.MRC_ERR_NOMEM and int(total[0]) == want["total"]
    full = np.zeros(int(total[0]), np.uint8)
    assert _lib.lib.mrc_chain_fetch_output(h._h, vp(full), full.size, P(total, _lib._i64p)) == 0
    assert full.tobytes() == want["bytes"].tobytes()
    assert np.array_equal(so, want["stream_offset"])


# ---------------------------------------------------------------- reservoir handover
def test_mono_reservoir_handover_at_block_boundary():
    codes, shapes, num = _streams(12, seed=3)
    s = int(np.argmax([len(sh) for sh in shapes]))
    sh = shapes[s]
    h = _handle()
    x = codes[s:s + 1]
    full = h.encode_chained_pac(x, None, [sh], with_flush=True, want_items=True)
    for k in (1, len(sh) // 2, len(sh) - 1):
        p1 = h.encode_chained_pac(x, None, [sh[:k]], with_flush=False)
        p2 = h.encode_chained_pac(x, None, [sh[k:]], with_flush=True, reservoir_in=p1["reservoir_out"])
        assert p1["bytes"].tobytes() + p2["bytes"].tobytes() == full["bytes"].tobytes(), "cut at block %d" % k
        assert p1["bytes"].size == full["item_offset"][k]
        assert int(p2["reservoir_out"][0]) == int(full["reservoir_out"][0])


# ---------------------------------------------------------------- sensitivity
def test_mono_certify(tmp_path):
    from mrcaudiocodec_amd import cli
    g = _fixture()
    wav = _write_wav(tmp_path, g["noise48_pcm"], int(g["noise48_rate"]))
    cert = {}
    got = cli.encode_wav(wav, None, certify=cert)
    assert cert["blocks_examined"] > 0
    assert cert["decisions_near_an_edge"] == 0
    assert got == cli.encode_wav(wav, None) == g["noise48_pac"].tobytes()


# ---------------------------------------------------------------- refusals
def test_mono_refusals(tmp_path):
    from mrcaudiocodec_amd import cli
    from mrcaudiocodec_amd._lib import MrcError
    h = _handle()
    codes = np.zeros((1, 6 * L), np.int16)
    codes[0, L:] = (np.arange(5 * L) % 200 - 100).astype(np.int16)
    with pytest.raises(MrcError):                                       # not one of the four shapes
        h.encode_chained_pac(codes, None, [[(0, L, L), (L, L, 512), (L + L, 512, L)]])
    with pytest.raises(MrcError):                                       # Close() needs a long last block
        h.encode_chained_pac(codes, None, [[(0, L, L), (L, L, 128)]], with_flush=True)
    with pytest.raises(ValueError, match="3-channel"):
        cli.encode_wav(_write_wav(tmp_path, np.zeros((3, 4 * L), np.int16), 48000), None)
    ok = h.encode_chained_pac(codes, None, [[(0, L, L), (L, L, L)]], with_flush=True)          # (the handle still works)
    assert ok["total"] > 0


# ---------------------------------------------------------------- stereo through the same entry points
def test_stereo_unchanged_through_same_entry_points():
    from mrcaudiocodec_amd import pacfile, transient
    h = _handle()
    rng = np.random.default_rng(21)
    n = 9 * L
    st = np.zeros((2, n + 3 * L), np.int16)
    x = rng.normal(0, 0.1 * 32767, (2, n))
    x[:, 4000:4128] *= 6
    st[:, L:L + n] = np.clip(np.rint(x), -32767, 32767)
    sh = transient.block_shape_array(h, st)
    assert sh[-1, 2] == L
    got = h.encode_chained_pac(st[0][None], st[1][None], [sh], num_samples=[n], want_items=True)
    want = pacfile.encode_stereo_stream_per_block(h, MO.to_float(st), [tuple(v) for v in sh.tolist()], num_samples=n)
    assert got["bytes"].tobytes() == want
    assert int.from_bytes(want[8:10], "little") == 2
    assert len(got["item_offset"]) == len(sh) + 2 + 1


# ---------------------------------------------------------------- sharded stream mode, mono
def test_shard_mono_streams_concatenate_to_one_call():
    from mrcaudiocodec_amd import pacfile, shard
    codes, shapes, num = _streams(20, seed=55)
    h = _handle()
    want = pacfile.encode_mono_streams(h, codes, shapes, num_samples=num)
    got = []
    for rank in range(3):
        first, files = shard.encode_streams_sharded(h, codes[:, None, :], shapes, 3, rank, num_samples=num)
        assert first == len(got)
        got += files
    assert got == want
    assert all(int.from_bytes(f[8:10], "little") == 1 for f in got)
