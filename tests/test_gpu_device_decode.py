"""
GPU tests of the device-side `.pac` decode: mrc_dev_unpack_blocks (the chunk parser on the device) against the host
parser integer for integer, accept / reject included, on the corpus and the seeded corruptions of tests/unpack_corpus.py;
mrc_decode_pac_pcm16 (whole files -> interleaved 16-bit PCM in one call) against the present path,
pacfile.decode_pac_pcm16 (host parser + per-shape device decode), and against the reference CLI's decoded WAVs.
"""
import ctypes as C

import numpy as np
import pytest

import refgold as G
import unpack_corpus as UC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def h():
    from mrcaudiocodec_amd import Handle
    hd = Handle()
    yield hd
    hd.close()


_HANDLES = {}


def _handle_for(cfg):
    from mrcaudiocodec_amd import Handle
    fields = ("sample_rate", "n_mdct_lines", "n_short", "n_scale_bits", "n_mant_size_bits", "blksw_bits_a", "blksw_bits_b")
    key = tuple(getattr(cfg, k) for k in fields)             # (setting E of the crafted cases: 3 scale bits, 5 size bits)
    if key not in _HANDLES:
        _HANDLES[key] = Handle(**dict(zip(fields, key)))
    return _HANDLES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for hd in _HANDLES.values():
        hd.close()
    _HANDLES.clear()


def _dev_parse(case, hd=None):
    """Handle.dev_unpack_blocks on device copies of the case -> dict of host arrays, or None if refused (hd: the handle to
    parse on; None: one of the case's rate and allocation-field width)"""
    from mrcaudiocodec_amd import MrcError
    hd = hd if hd is not None else _handle_for(case["cfg"])
    dev = torch.device("cuda", 0)
    nch, joint, L = case["nch"], case["joint"], case["cfg"].n_mdct_lines
    offs = np.ascontiguousarray(case["offsets"], np.int64)
    n = offs.size // nch
    buf = torch.from_numpy(np.frombuffer(case["buf"], np.uint8).copy()).to(dev)
    doffs = torch.from_numpy(offs).to(dev)
    shapes = dict(a=(n,), b=(n,), huff_table=(n, nch), overall_scale=(n, 4 if joint else nch), ms_switch=(n, 32),
                  scale_factor=(n, nch, 32), bit_alloc=(n, nch, 32), mantissa=(n, nch, L))
    out = {k: torch.zeros(s, dtype=torch.int32, device=dev) for k, s in shapes.items()}
    p = lambda k: out[k].data_ptr()
    try:
        hd.dev_unpack_blocks(n, nch, joint, buf.data_ptr(), buf.numel(), doffs.data_ptr(), p("a"), p("b"), p("huff_table"),
                             p("overall_scale"), p("ms_switch"), p("scale_factor"), p("bit_alloc"), p("mantissa"))
    except MrcError as e:
        assert e.code == -1, e
        return None
    return {k: v.cpu().numpy() for k, v in out.items()}


def _compare(cases, hd=None):
    n_acc = n_rej = 0
    for c in cases:
        want, got = UC.host_parse(c), _dev_parse(c, hd)
        if want is None:
            assert got is None, "%s: the host parser refuses, the device accepts" % c["label"]
            n_rej += 1
            continue
        assert got is not None, "%s: the host parser accepts, the device refuses" % c["label"]
        for k, v in want.items():
            if k == "ms_switch" and not c["joint"]:
                continue
            assert np.array_equal(got[k], v), "%s: %s differs" % (c["label"], k)
        n_acc += 1
    return n_acc, n_rej


def test_dev_unpack_equals_host_parser_on_corpus():
    bases = UC.base_cases()
    n_acc, n_rej = _compare(bases)
    assert n_rej == 0 and n_acc == len(bases) >= 144                         # (the crafted decode cases among them)
    assert sum(c["label"].startswith("crafted_") for c in bases) == 36


def test_dev_unpack_agrees_on_damaged_chunks():
    damaged = UC.corruptions(UC.base_cases(), n=2000)
    n_acc, n_rej = _compare(damaged)
    assert n_rej >= 500 and n_acc >= 100, (n_acc, n_rej)
    # the device is still well after two thousand refusals and acceptances
    assert _compare(UC.base_cases()[:2]) == (2, 0)


# ------------------------------------------------------------------------------------------------ whole files
def _files_equal_present_path(hd, files, skip=()):
    """skip: files the present path cannot take (a header without chunks: it hands mrc_dev_pcm16 an empty tensor)"""
    from mrcaudiocodec_amd import pacfile as ppac
    got = ppac.decode_pac_files(hd, files)
    assert len(got) == len(files)
    for i, (f, g) in enumerate(zip(files, got)):
        if i in skip:
            continue
        want = ppac.decode_pac_pcm16(hd, f)
        assert g.dtype == np.int16 and g.shape == want.shape, (i, g.shape, want.shape)
        assert np.array_equal(g, want), "file %d differs from the present path" % i
    return got


@pytest.mark.parametrize("case", ["a48", "b44"])
def test_decode_pac_files_equal_reference_cli(case):
    from mrcaudiocodec_amd import Handle, pacfile as ppac
    g = G.load("ref_pac.npz")
    for which in ("_pac", "_pac_raw"):
        buf = g[case + which].tobytes()
        cfg, _, _, _ = ppac.read_header(buf)
        hd = Handle(sample_rate=cfg.sample_rate)
        try:
            pcm = _files_equal_present_path(hd, [buf])[0]
        finally:
            hd.close()
        if which == "_pac":
            want = g[case + "_decoded"]    # its first 1024 samples are the reference driver's stale look-ahead block
            assert np.array_equal(pcm[:, :want.shape[1] - 1024], want[:, 1024:])


def test_cli_decode_writes_the_present_paths_wav(tmp_path):
    from mrcaudiocodec_amd import Handle, cli, pacfile as ppac
    g = G.load("ref_pac.npz")
    for case in ("a48", "b44"):
        buf = g[case + "_pac"].tobytes()
        path = str(tmp_path / (case + ".pac"))
        with open(path, "wb") as f:
            f.write(buf)
        cli.main(["-d", path, str(tmp_path / (case + ".wav"))])
        cfg, _, _, _ = ppac.read_header(buf)
        hd = Handle(sample_rate=cfg.sample_rate)
        try:
            want = cli.wav_bytes(ppac.decode_pac_pcm16(hd, buf), cfg.sample_rate)
        finally:
            hd.close()
        assert open(str(tmp_path / (case + ".wav")), "rb").read() == want


def _switched_pcm(hops, period, seed):
    rng = np.random.default_rng(seed)
    n = hops * 1024
    t = np.arange(n)
    g1, g2 = rng.normal(0, 0.02 * 32767, n), rng.normal(0, 0.02 * 32767, n)
    tone = 0.2 * 32767 * np.sin(2 * np.pi * 440.0 * t / 48000)
    left, right = g1 + tone, 0.7 * g1 + 0.3 * g2 + 0.9 * tone
    for k in range(period - 1, hops, period):
        burst = rng.normal(0, 0.5 * 32767, 128)
        left[k * 1024:k * 1024 + 128] = burst
        right[k * 1024:k * 1024 + 128] = 0.8 * burst
    pcm = np.zeros((2, (hops + 1) * 1024), np.int16)
    pcm[0, 1024:] = np.clip(np.rint(left), -32767, 32767)
    pcm[1, 1024:] = np.clip(np.rint(right), -32767, 32767)
    return pcm


def _switched_file(hd, hops, period=37, seed=42):
    from mrcaudiocodec_amd import synth, transient
    pcm = _switched_pcm(hops, period, seed)
    shapes = transient.block_shapes(hd, synth.pcm_to_float(pcm))
    while shapes and shapes[-1][2] != 1024:
        shapes.pop()
    r = hd.encode_chained_pac(pcm[0][None], pcm[1][None], [shapes], num_samples=[sum(b for (_, _, b) in shapes)])
    return r["bytes"].tobytes(), shapes


def test_switched_stream_of_4096_hops(h):
    buf, shapes = _switched_file(h, 4096)
    assert len({(a, b) for (_, a, b) in shapes}) == 4                 # every block shape occurs
    pcm = _files_equal_present_path(h, [buf])[0]
    assert pcm.shape[0] == 2 and pcm.shape[1] > 4000 * 1024


def _mixed_files(h):
    from mrcaudiocodec_amd import pacfile as ppac, synth
    from oracle import fast
    cfg = ppac.make_config()
    rng = np.random.default_rng(3)
    n_streams, hop = 60, 1024
    pl = np.clip(np.rint(rng.normal(0, 3000, (n_streams, 13 * hop))), -32767, 32767)
    pl[:, :hop] = 0
    pr = np.clip(np.rint(0.7 * pl + 0.3 * np.roll(pl, 17, axis=1)), -32767, 32767)
    shapes = [[(i * hop, hop, hop) for i in range(1 + s % 12)] for s in range(n_streams)]   # 1..12 blocks + Close()
    files = ppac.encode_stereo_streams(h, np.stack([pl, pr], axis=1).astype(np.int16), shapes)
    # one stereo file of a single block: both chunks through the non-joint reader
    osc, sw, sf, ba, mant = UC._random_blocks(cfg, hop, hop, 1, 2, rng)
    d, _, _, _ = ppac.pack_blocks(cfg, hop, hop, osc[:, :2], sf, ba, mant, True)
    single = ppac.header(cfg, 2, hop) + d.tobytes()
    # one mono file (WriteDataBlock chunks)
    x = synth.c1_sine(9)
    enc = h.encode_mono(np.array(fast.blocks_from_stream(x, hop)), hop, hop)
    d, _, _, _ = ppac.pack_blocks(cfg, hop, hop, enc["overall_scale"][:, None], enc["scale_factor"][:, None, :],
                                  enc["bit_alloc"][:, None, :], enc["mantissa"][:, None, :], True)
    mono = ppac.header(cfg, 1, 8 * hop) + d.tobytes()
    empty = ppac.header(cfg, 2, 0)                                    # a header and no chunks
    switched, _ = _switched_file(h, 40, period=7, seed=9)
    mixed = files[:30] + [single, mono] + files[30:45] + [empty, switched] + files[45:]
    return mixed, mixed.index(empty)


def test_many_mixed_files_in_one_call(h):
    files, empty = _mixed_files(h)
    assert len(files) == 64
    got = _files_equal_present_path(h, files, skip=(empty,))
    assert got[empty].shape == (2, 0)
    assert [g.shape[0] for g in got].count(1) == 1
    inter = h.decode_pac_pcm16(files)                                # WAV order: [samples][nCh], the same values
    for g, i in zip(got, inter):
        assert np.array_equal(g.T, i)
    ms = h.decode_ms()
    assert ms.shape == (4,) and (ms > 0).all()


def test_short_output_buffer_reports_the_size_needed(h):
    from mrcaudiocodec_amd import _lib
    files = _mixed_files(h)[0][:5]
    data = np.frombuffer(b"".join(files), np.uint8)
    fo = np.zeros(len(files) + 1, np.int64)
    fo[1:] = np.cumsum([len(f) for f in files])
    so = np.zeros(len(files) + 1, np.int64)
    nch = np.zeros(len(files), np.int32)
    need = sum(g.size for g in h.decode_pac_pcm16(files))
    out = np.full(need, 12345, np.int16)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = _lib.lib.mrc_decode_pac_pcm16(h._h, len(files), vp(data), vp(fo), vp(out), need - 1, vp(so), vp(nch))
    assert rc == _lib.MRC_ERR_NOMEM
    assert so[-1] == need and (out == 12345).all()
    assert list(nch) == [2] * 5
    rc = _lib.lib.mrc_decode_pac_pcm16(h._h, len(files), vp(data), vp(fo), vp(out), need, vp(so), vp(nch))
    assert rc == 0 and so[-1] == need
    assert np.array_equal(out, np.concatenate([g.reshape(-1) for g in h.decode_pac_pcm16(files)]))


def test_file_parameters_must_match_the_handle(h):
    from mrcaudiocodec_amd import MrcError, pacfile as ppac
    g = G.load("ref_pac.npz")
    ok = g["a48_pac"].tobytes()
    with pytest.raises(MrcError, match="sample_rate"):
        h.decode_pac_pcm16([ok, g["b44_pac"].tobytes()])            # 44.1 kHz file, 48 kHz handle
    cfg5 = ppac.make_config(n_mant_size_bits=5)
    with pytest.raises(MrcError, match="n_mant_size_bits"):
        h.decode_pac_pcm16(ppac.header(cfg5, 2, 0))
    assert np.array_equal(ppac.decode_pac_files(h, [ok])[0], ppac.decode_pac_pcm16(h, ok))


def test_damaged_file_is_a_clean_error(h):
    from mrcaudiocodec_amd import MrcError, pacfile as ppac
    g = G.load("ref_pac.npz")
    ok = g["a48_pac"].tobytes()
    cfg, _, _, off = ppac.read_header(ok)
    chunks = ppac.scan_chunks(ok, off)
    bad = bytearray(ok)
    bad[chunks[3] + 4] = (bad[chunks[3] + 4] & 0x0F) | 0x90         # table id 9
    with pytest.raises(MrcError, match="table id"):
        h.decode_pac_pcm16([ok, bytes(bad)])
    with pytest.raises(MrcError):
        h.decode_pac_pcm16(ok[:-5])                                   # truncated last chunk
    assert np.array_equal(ppac.decode_pac_files(h, [ok])[0], ppac.decode_pac_pcm16(h, ok))
