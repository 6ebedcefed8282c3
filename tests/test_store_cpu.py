"""
Host side of the resident `.pac` store, no GPU: mrc_pac_index / pacfile.index against a restatement from the calls that
existed before it (read_header, scan_chunks, unpack_blocks) on the reference's own files, the sizing protocol, the refusals
with their texts, the ctypes binding of the six new functions against the header, and the command line's refusals of
--start / --samples.
"""
import ctypes as C

import numpy as np
import pytest

import chain_kit as kit
import refgold as G

NAMES = ("mrc_pac_index", "mrc_pac_store_create", "mrc_pac_store_destroy", "mrc_pac_store_info",
         "mrc_pac_store_decode_window", "mrc_pac_store_stats")
FILES = (("a48_pac", 35), ("a48_pac_raw", 35), ("b44_pac", 33), ("b44_pac_raw", 33))


def _file(key):
    return G.load("ref_pac.npz")[key].tobytes()


def _restated(buf):
    """(a, b) per block and the chunk offsets from the parser that reads whole chunks"""
    from mrcaudiocodec_amd import pacfile as ppac
    cfg, nch, _, off = ppac.read_header(buf)
    chunks = ppac.scan_chunks(buf, off)
    n = len(chunks) // nch
    if nch == 2 and n > 1:
        parts = [ppac.unpack_blocks(cfg, buf, chunks[:2 * (n - 1)], 2, True), ppac.unpack_blocks(cfg, buf, chunks[2 * (n - 1):], 2, False)]
    else:
        parts = [ppac.unpack_blocks(cfg, buf, chunks, nch, False)]
    return nch, chunks, np.concatenate([p["a"] for p in parts]), np.concatenate([p["b"] for p in parts])


@pytest.mark.parametrize("key,n_blocks", FILES)
def test_index_equals_the_restatement(key, n_blocks):
    from mrcaudiocodec_amd import pacfile as ppac
    buf = _file(key)
    nch, chunks, a, b = _restated(buf)
    ix = ppac.index(buf)
    assert ix["n_channels"] == nch == 2 and ix["n_blocks"] == n_blocks == len(a)
    assert np.array_equal(ix["chunk_offset"], chunks.reshape(n_blocks, nch))
    assert np.array_equal(ix["block_a"], a) and np.array_equal(ix["block_b"], b)
    assert np.array_equal(ix["block_start"], np.concatenate([[0], np.cumsum(a)[:-1]]))
    assert ix["n_samples"] == ix["block_start"][-1] + a[-1] + b[-1] - 1024
    assert {(int(x), int(y)) for x, y in zip(a, b)} == {(1024, 1024), (1024, 128), (128, 128), (128, 1024)}


def _raw_index(buf, cap, cfg=None, arrays=True):
    from mrcaudiocodec_amd import _lib, pacfile as ppac
    raw = np.frombuffer(buf, np.uint8)
    cfg = cfg or ppac.read_header(buf)[0]
    nch, nb, ns = C.c_int32(-7), C.c_int64(-7), C.c_int64(-7)
    out = [np.full(max(cap, 1), -7, np.int64), np.full(max(cap, 1), -7, np.int32), np.full(max(cap, 1), -7, np.int32),
           np.full(2 * max(cap, 1), -7, np.int64)]
    ptr = [o.ctypes.data if arrays else None for o in out]
    rc = _lib.lib.mrc_pac_index(C.byref(cfg), raw.ctypes.data, raw.size, C.byref(nch), C.byref(nb), C.byref(ns), cap, *ptr)
    return rc, nch.value, nb.value, ns.value, out


def test_sizing_protocol_leaves_the_arrays_untouched():
    from mrcaudiocodec_amd import _lib
    buf = _file("a48_pac")
    for cap, arrays in ((34, True), (0, True), (35, False)):
        rc, nch, nb, ns, out = _raw_index(buf, cap, arrays=arrays)
        assert rc == _lib.MRC_ERR_NOMEM and (nch, nb, ns) == (2, 35, 14336)
        assert all((o == -7).all() for o in out)
    rc, nch, nb, ns, out = _raw_index(buf, 35)
    assert rc == 0 and (nch, nb, ns) == (2, 35, 14336) and out[0][0] == 0 and out[0][34] == ns + 1024 - 2048


def _refused(buf, match, cfg=None):
    from mrcaudiocodec_amd import MrcError, pacfile as ppac
    with pytest.raises(MrcError, match=match):
        ppac.index(buf, cfg)


def test_refusals_and_their_texts():
    from mrcaudiocodec_amd import pacfile as ppac
    buf = _file("a48_pac")
    _, _, _, data_offset = ppac.read_header(buf)
    chunks = ppac.scan_chunks(buf, data_offset)
    _refused(buf[:int(chunks[7]) + 9], r"mrc_pac_index: file 0: truncated chunk at byte %d" % chunks[7])
    _refused(buf[:int(chunks[-1])], r"mrc_pac_index: file 0: 69 chunks for 2 channels")
    _refused(buf, r"mrc_pac_index: file 0 has sample_rate = 48000, cfg has 44100", ppac.make_config(sample_rate=44100))
    _refused(buf[:10], r"mrc_pac_index: file 0: not a \.pac header", ppac.make_config())
    ix = ppac.index(buf[:data_offset])                      # a header alone
    assert (ix["n_channels"], ix["n_blocks"], ix["n_samples"]) == (2, 0, 0) and ix["block_start"].size == 0
    assert ix["chunk_offset"].shape == (0, 2)


def test_the_whole_file_decode_keeps_its_texts():
    """the scan that mrc_pac_index shares with mrc_decode_pac_pcm16 words the handle's refusals as before: the one text a
    CPU can reach is asserted here on the source, the others by the GPU tests of the whole-file decode"""
    import os
    src = open(os.path.join(kit.ROOT, "mrcaudiocodec_amd", "csrc", "mrc_api_decode.cpp")).read()
    assert src.count("truncated chunk at byte") == 1 and src.count("mrc_pac_read_header(") == 1     # one scan in the tree
    assert '"the handle was created with"' in src and '"%s: file %lld has %s = %d, %s %d"' in src


def test_binding_of_the_store_calls():
    kit.check_binding(NAMES)
    from mrcaudiocodec_amd import _lib
    text = kit.header_text()
    for name, value in (("MRC_WINDOW_PCM16", 0), ("MRC_WINDOW_F32", 1), ("MRC_WINDOW_F64", 2), ("MRC_OPT_STORE_SLAB_SAMPLES", 7)):
        assert getattr(_lib, name) == value and ("#define %s %d" % (name, value)) in " ".join(text.split())


@pytest.mark.parametrize("argv,text", [
    (["in.wav", "out.pac", "--start", "5"], "they need -d"),
    (["in.wav", "out.pac", "--samples", "5"], "they need -d"),
    (["in.wav", "out.pac", "--start", "0", "--samples", "5"], "they need -d"),
    (["-d", "in.pac", "out.wav", "--samples", "-1"], "is negative"),
])
def test_cli_refuses_an_excerpt_that_makes_no_sense(argv, text, capsys):
    from mrcaudiocodec_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2 and text in capsys.readouterr().err


def test_cli_excerpt_defaults():
    from mrcaudiocodec_amd import cli
    assert cli.check_excerpt_args(None, None, True) is None and cli.check_excerpt_args(None, None, False) is None
    assert cli.check_excerpt_args(7, None, True) == (7, None)           # to the end
    assert cli.check_excerpt_args(None, 9, True) == (0, 9)
    assert cli.check_excerpt_args(-3, 0, True) == (-3, 0)
