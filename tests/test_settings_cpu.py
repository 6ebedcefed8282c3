"""
CPU tests of the file layer at the codec settings of tests/settings_kit.py: the kit's own inputs (conditions on the oracle
alone), the host packer against the oracle's writer and the host parser against the oracle's parser at every setting and
block shape (raw, priced and forced Huffman tables), the header writer / reader / index round trip, and the portable chunk
parser (the code the device runs) on the settings' chunks and seeded corruptions of them.
"""
import struct

import numpy as np
import pytest

import mono_oracle
import settings_kit as SK
import test_unpack_portable as TP
import unpack_corpus as UC
from mrcaudiocodec_amd import pacfile as ppac
from oracle import decode as odec, pacfile as opac

FILES = [(nch, huff) for nch in (2, 1) for huff in (True, False)]


# ------------------------------------------------------------------ the kit itself, on the oracle alone
def test_every_setting_covers_something():
    assert sorted(SK.COVERS) == SK.IDS == list("BCDEFGHIJK")
    for sid in SK.IDS:
        assert SK.COVERS[sid], sid
        assert {1, 2, 4, 5, 7} <= SK.COVERS[sid], sid
    assert all(3 in SK.COVERS[s] for s in "BEFH") and all(6 in SK.COVERS[s] for s in "BCDK") and 9 in SK.COVERS["J"]
    assert all(8 in SK.COVERS[s] for s in "BCFH")
    assert set(SK.HUFFMAN_FORCED) <= set(SK.IDS)


@pytest.mark.parametrize("sid", SK.IDS)
def test_kit_inputs_meet_their_conditions(sid):
    L, S = SK.lengths(sid)
    pcm = SK.stream(sid)
    assert pcm.dtype == np.int16 and pcm.shape == (2, (SK.n_hops(sid) + 1) * L) and not pcm[:, :L].any()
    for which in (0, 1):
        sch = SK.schedule(sid, which)
        assert 6 <= len(sch) + 1 <= 14 and sch[-1][1:] == (L, L) and sch[0][1:] == (L, L)
        assert sch[-1][0] + 2 * L <= pcm.shape[1]
        assert all(o2 == o1 + a1 and a2 == b1 for (o1, a1, b1), (o2, a2, _) in zip(sch, sch[1:]))      # the blocks chain
        assert {(a, b) for _, a, b in sch} == set(SK.shapes_of(sid))
    assert SK.schedule(sid, 0) != SK.schedule(sid, 1)
    x = SK.to_float(pcm)
    for nch, huff in FILES:
        f = SK.oracle_file(sid, nch, huff)
        # the kit's block-by-block spelling is the oracle's own writer
        if nch == 2:
            want = opac.encode_stereo_stream(x, SK.schedule(sid), cp=SK.coding_params(sid, 2), huffman=huff)
        else:
            want = mono_oracle.encode_mono_stream(x[:1], SK.schedule(sid), cp=SK.coding_params(sid, 1), huffman=huff)
        assert f["data"] == want
        assert {(b["a"], b["b"]) for b in f["blocks"]} == set(SK.shapes_of(sid))
        if nch == 2:
            ms = np.concatenate([b["ms"] for b in f["blocks"] if b["joint"]])
            assert (ms == 1).any() and (ms == 0).any(), "M/S switch never %s" % ("set" if not ms.any() else "cleared")
        tabs = [t for b in f["blocks"] for t in b["table"]]
        if huff and sid not in SK.HUFFMAN_FORCED:
            assert any(t in (0, 1, 2, 3) for t in tabs) and any(t == 15 for t in tabs), tabs
        if not huff:
            assert set(tabs) == {15}
    if sid == "F":
        f = SK.oracle_file(sid, 1, False)
        assert min(int(np.min(s)) for b in f["blocks"] for s in b["sf"]) == -1       # an empty band at one scale bit


# ------------------------------------------------------------------ host packer / parser against the oracle's
def _groups(blocks):
    out = {}
    for i, b in enumerate(blocks):
        out.setdefault((b["a"], b["b"], b["joint"], b["nch"]), []).append(i)
    return out


@pytest.mark.parametrize("sid", SK.IDS)
def test_host_packer_equals_the_oracle_writer(sid):
    cfg = SK.config(sid)
    for nch, huff in FILES:
        f = SK.oracle_file(sid, nch, huff)
        for (a, b, joint, n_ind), idx in _groups(f["blocks"]).items():
            blocks = [f["blocks"][i] for i in idx]
            osc, ms, sf, ba, mant = SK.block_arrays(blocks)
            want_tab = np.array([bl["table"] for bl in blocks], np.int32)
            pack = (lambda **kw: ppac.pack_joint_blocks(cfg, a, b, osc, ms, sf, ba, mant, **kw)) if joint else \
                (lambda **kw: ppac.pack_blocks(cfg, a, b, osc, sf, ba, mant, **kw))
            data, offs, table, _ = pack(use_huffman=huff)                   # priced by the host (or raw)
            assert np.array_equal(table, want_tab), (sid, nch, huff, a, b)
            for k, bl in enumerate(blocks):
                assert data[offs[k]:offs[k + 1]].tobytes() == bl["chunk"], (sid, nch, huff, a, b, k)
            given = pack(huff_table=want_tab)                               # the tables given
            assert given[0].tobytes() == data.tobytes()


def _payloads(buf, offsets):
    return [buf[int(o) + 4:int(o) + 4 + struct.unpack("<L", buf[int(o):int(o) + 4])[0]] for o in offsets]


def _oracle_parse(sid, case):
    """oracle.decode.parse_block / parse_joint_block over a chunk-parser case -> the arrays of pacfile.unpack_blocks"""
    nch, joint = case["nch"], case["joint"]
    cp = SK.coding_params(sid, nch)
    chunks = _payloads(case["buf"], case["offsets"])
    n = len(chunks) // nch
    L = cp.nMDCTLines
    out = dict(a=np.zeros(n, np.int32), b=np.zeros(n, np.int32), huff_table=np.zeros((n, nch), np.int32),
               overall_scale=np.zeros((n, 4 if joint else nch), np.int32), ms_switch=np.zeros((n, 32), np.int32),
               scale_factor=np.zeros((n, nch, 32), np.int32), bit_alloc=np.zeros((n, nch, 32), np.int32),
               mantissa=np.zeros((n, nch, L), np.int32))
    for i in range(n):
        if joint:
            p = odec.parse_joint_block(chunks[2 * i], chunks[2 * i + 1], cp)
            parts = [dict(huffTable=p["huffTable"][c], scaleFactor=p["scaleFactor"][c], bitAlloc=p["bitAlloc"][c],
                          mantissa=p["mantissa"][c]) for c in range(2)]
            out["overall_scale"][i] = p["overallScale"]
            out["ms_switch"][i, :len(p["ms_switch"])] = p["ms_switch"]
        else:
            parts = [odec.parse_block(chunks[nch * i + c], cp) for c in range(nch)]
            out["overall_scale"][i] = [q["overallScale"] for q in parts]
        out["a"][i], out["b"][i] = cp.a, cp.b
        for c, q in enumerate(parts):
            nb = len(q["bitAlloc"])
            out["huff_table"][i, c] = q["huffTable"]
            out["scale_factor"][i, c, :nb] = q["scaleFactor"]
            out["bit_alloc"][i, c, :nb] = q["bitAlloc"]
            out["mantissa"][i, c] = q["mantissa"]
    return out


@pytest.mark.parametrize("sid", SK.IDS)
def test_host_parser_equals_the_oracle_parser(sid):
    cases = SK.file_cases(sid) + SK.forced_table_cases(sid)
    assert {int(t) for c in cases for t in UC.host_parse(c)["huff_table"].ravel()} == {0, 1, 2, 3, 15}
    for case in cases:
        got, want = UC.host_parse(case), _oracle_parse(sid, case)
        assert got is not None, case["label"]
        for k, v in want.items():
            if k == "ms_switch" and not case["joint"]:
                continue
            assert np.array_equal(got[k], v), (case["label"], k)
    # the integers the oracle WROTE come back (a scale factor of -1 as its low bits)
    mask = (1 << SK.full(sid)["n_scale_bits"]) - 1
    for nch, huff in FILES:
        f = SK.oracle_file(sid, nch, huff)
        for case in UC._file_cases(f["data"], "x", SK.config(sid)):
            got = UC.host_parse(case)
            blocks = [b for b in f["blocks"] if b["joint"] == case["joint"]]
            assert len(blocks) == len(got["a"])
            for i, bl in enumerate(blocks):
                nb, half = bl["bands"].nBands, (bl["a"] + bl["b"]) // 2
                assert (got["a"][i], got["b"][i]) == (bl["a"], bl["b"]) and list(got["huff_table"][i]) == bl["table"]
                assert list(got["overall_scale"][i]) == bl["os"]
                for c in range(nch):
                    assert np.array_equal(got["scale_factor"][i, c, :nb], np.asarray(bl["sf"][c]) & mask)
                    assert np.array_equal(got["bit_alloc"][i, c, :nb], bl["ba"][c])
                    assert np.array_equal(got["mantissa"][i, c, :half], bl["mant"][c])
                if bl["joint"]:
                    assert np.array_equal(got["ms_switch"][i, :nb], bl["ms"])


@pytest.mark.parametrize("sid", SK.IDS)
def test_oracle_files_round_trip_through_the_oracle(sid):
    """the parameterised oracle decoder reads what the oracle's encoder wrote at the setting: the signal comes back"""
    L, S = SK.lengths(sid)
    for nch in (2, 1):
        f = SK.oracle_file(sid, nch, True)
        x = SK.oracle_decode(sid, f["data"])
        src = SK.to_float(SK.source(sid, nch))
        assert x.shape == (nch, src.shape[1] + 2 * L)
        err = x[:, L:L + src.shape[1]] - src
        # no bar on the codec (one scale bit leaves 3 dB): the blocks landed where the signal is, so the error is below it
        assert np.isfinite(x).all() and np.mean(err ** 2) < np.mean(src ** 2)
    if sid not in ("J",) and (S != 128 or SK.blksw(sid) != (1, 1)):
        with pytest.raises(Exception):                          # the reference's literals cannot read this file
            odec.decode_pac(SK.oracle_file(sid, 2, True)["data"])


# ------------------------------------------------------------------ header writer, reader and index
@pytest.mark.parametrize("sid", SK.IDS)
def test_header_round_trip(sid):
    cfg, f = SK.config(sid), SK.full(sid)
    L, S = SK.lengths(sid)
    for nch in (1, 2):
        for n in (5000, 4 * L, 0):
            head = ppac.header(cfg, nch, n)
            assert head == opac.file_header(SK.coding_params(sid, nch), n)
            got, got_nch, got_n, off = ppac.read_header(head)
            assert (got_nch, off) == (nch, len(head)) and got_n == (n + L if n % L == 0 else n)
            for k in ("sample_rate", "n_mdct_lines", "n_scale_bits", "n_mant_size_bits"):
                assert getattr(got, k) == f[k], k
        file = SK.oracle_file(sid, nch, True)
        ix = ppac.index(file["data"], cfg)
        sch = file["shapes"]
        assert ix["n_channels"] == nch and ix["n_blocks"] == len(sch) + 1
        assert ix["block_a"].tolist() == [a for _, a, _ in sch] + [L] and ix["block_b"].tolist() == [b for _, _, b in sch] + [L]
        assert ix["block_start"].tolist() == [o for o, _, _ in sch] + [sch[-1][0] + sch[-1][1]]
        assert ix["n_samples"] == sum(b for _, _, b in sch) + L
        assert ix["chunk_offset"][0, 0] == len(ppac.header(cfg, nch, 0))


@pytest.mark.parametrize("L,ok", [(1024, True), (768, True), (576, True), (384, True), (96, True), (16, True), (8192, True),
                                  (6144, True), (640, False), (1000, False), (1022, False), (729, False), (8, False),
                                  (8193, False), (12288, False)])
def test_header_reader_accepts_what_a_handle_can_write(L, ok):
    """16 <= n_mdct_lines <= 8192, even, no prime factor but 2 and 3 (build_shape's rule for (L, L)); else refused"""
    head = bytearray(ppac.header(ppac.make_config(), 2, 5000))
    head[14:18] = struct.pack("<L", L)
    if ok:
        assert ppac.read_header(bytes(head))[0].n_mdct_lines == L
    else:
        with pytest.raises(ppac.MrcError, match="header field out of range"):
            ppac.read_header(bytes(head))
    for at, bad in ((8, struct.pack("<H", 3)), (18, struct.pack("<H", 5)), (20, struct.pack("<H", 9)), (4, struct.pack("<L", 0))):
        damaged = bytearray(ppac.header(ppac.make_config(n_mdct_lines=768, n_short=384), 2, 5000))
        damaged[at:at + len(bad)] = bad
        with pytest.raises(ppac.MrcError, match="header field out of range"):      # every other refusal stays
            ppac.read_header(bytes(damaged))


# ------------------------------------------------------------------ the portable parser (what the device runs)
def settings_cases():
    out = []
    for sid in SK.IDS:
        out += SK.file_cases(sid) + SK.forced_table_cases(sid)
    return out


def test_portable_parser_on_the_settings(tmp_path):
    cases = settings_cases()
    n_acc, n_rej, _ = TP._check(cases, tmp_path)
    assert n_rej == 0 and n_acc == len(cases) >= 10 * (6 + 10)
    (tmp_path / "damaged").mkdir()
    damaged = UC.corruptions(cases, n=3000, seed=17)
    n_acc, n_rej, sanitized = TP._check(damaged, tmp_path / "damaged")
    for sid in SK.IDS:
        assert sum(c["label"].startswith(sid + "_") for c in damaged) >= 100, sid
    assert n_rej >= 500 and n_acc >= 100, (n_acc, n_rej)
    print("settings: %d damaged chunk sets accepted, %d refused by both parsers; sanitizers %s" %
          (n_acc, n_rej, "on" if sanitized else "not available"))


def test_short_block_without_switch_bits_is_refused_by_the_host_parser():
    """block-switch width 0: the writer emits a short block, nothing in the chunk says so, the parser reads it as a long one
    and runs out of payload"""
    cfg = SK.config("J")
    L, S = SK.lengths("J")
    rng = np.random.default_rng(3)
    for (a, b) in ((L, S), (S, S), (S, L)):
        osc, sw, sf, ba, mant = UC._random_blocks(cfg, a, b, 2, 2, rng)
        ba[:] = 0                                              # the fewest bits: certainly shorter than a long block's chunk
        mant[:] = 0
        head = ppac.header(cfg, 2, 2 * b)
        blob = head + ppac.pack_joint_blocks(cfg, a, b, osc, sw, sf, ba, mant, False)[0].tobytes()
        case = dict(cfg=cfg, buf=blob, offsets=ppac.scan_chunks(blob, len(head)), nch=2, joint=True)
        assert UC.host_parse(case) is None
        with pytest.raises(ppac.MrcError, match=r"chunk at byte %d: read past the end of a chunk$" % len(head)):
            ppac.unpack_blocks(cfg, blob, case["offsets"], 2, True)
