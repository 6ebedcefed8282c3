"""
GPU tests of the `.pac` file layer on crafted codes (tests/pack_cases.py), held DIRECTLY against the oracle
(oracle.codec.calculateHuffmanGain, oracle.pacfile.pack_block / pack_joint_block) -- not against the host packer, which
shares the emit table and the lut_index rule with the device:

  huffman_gain_kernel     StreamEncoder.huffman_gain at one and two streams per block: table, bits_saved, reservoir_next
  pack_plan_kernel        the device packer pricing for itself, raw, and with the tables given
  pack_write_kernel       fast16 and the generic path (576 and 128 lines, bands without lines, 1024 lines on planes that are
                          not 16-byte aligned), both mantissa formats, batches of 1, 3, 4, 5 and all blocks, out_cap exact
  pack_scan_*             2051 mono and 1537 joint blocks: three scan tiles, a block start on every tile boundary
  unpack_fixed_kernel     Handle.dev_unpack_blocks on the oracle's bytes: the crafted integers come back

Every comparison is integer or byte equality; a failure names the case and the first differing byte or field.
"""
import numpy as np
import pytest

import pack_cases as pc

pytestmark = pytest.mark.gpu

IDS = [pc.config_id(c) for c in pc.CONFIGS]
LONG = [c for c in pc.CONFIGS if c[3] == c[4] == 1024]
CANARY, N_CANARY = 0xA5, 64


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def encoders(torch):
    from mrcaudiocodec_amd.batch import StreamEncoder
    encs = {k: StreamEncoder(device_id=0, sample_rate=k[0], n_scale_bits=k[1], n_mant_size_bits=k[2])
            for k in sorted({c[:3] for c in pc.CONFIGS})}
    yield encs
    for e in encs.values():
        e.h.close()


def _dev(torch, arr, dtype=None):
    t = torch.as_tensor(np.array(arr), device="cuda:0")                  # (a copy: the kit's arrays stay untouched)
    return t if dtype is None else t.to(dtype).contiguous()


def _inputs(torch, cfg, m16=False, index=None, offset=False):
    """the blocks of the configuration (or those of `index`) as StreamEncoder.encode would deliver them.  offset: the mantissa
    plane starts one element past a 16-byte boundary"""
    c = pc.cases(cfg)
    pick = (lambda x: x) if index is None else (lambda x: x[index])
    mant = pick(c["mantissa"])
    mant = mant.astype(np.uint16).view(np.int16) if m16 else mant
    if offset:
        buf = torch.zeros((mant.size + 1,), dtype=torch.int16 if m16 else torch.int32, device="cuda:0")
        dm = buf[1:].view(mant.shape)
        dm.copy_(_dev(torch, mant))
        assert dm.data_ptr() % 16 == (2 if m16 else 4) and dm.is_contiguous()
    else:
        dm = _dev(torch, mant)
    out = {"overall_scale": _dev(torch, pick(c["overall_scale"])), "scale_factor": _dev(torch, pick(c["scale_factor"])),
           "bit_alloc": _dev(torch, pick(c["bit_alloc"])), "mantissa": dm}
    if c["ms_switch"] is not None:
        out["ms_switch"] = _dev(torch, pick(c["ms_switch"]))
    return out


def _want(cfg, variant, n=None):
    """the oracle's (image, offsets, table, bits_saved or None) of the first n blocks"""
    e = pc.expected(cfg)
    n = len(e["blocks"][variant]) if n is None else n
    offs = e["offsets"][variant][:n + 1]
    saved = {"priced": e["bits_saved"][:n], "raw": np.zeros_like(e["bits_saved"][:n]), "forced": None}[variant]
    return e["image"][variant][:offs[-1]], offs, e["table"][variant][:n], saved


def _check(cfg, variant, got_bytes, got_offs, got_table, got_saved, want, what):
    image, offs, table, saved = want
    names = pc.cases(cfg)["names"]
    where = "%s %s %s" % (pc.config_id(cfg), variant, what)
    bad = np.argwhere(np.asarray(got_table) != table)
    assert not len(bad), "%s: table of %r is %d, the oracle chooses %d" % (
        where, names[bad[0][0]][bad[0][1]], np.asarray(got_table)[tuple(bad[0])], table[tuple(bad[0])])
    if saved is not None:
        bad = np.argwhere(np.asarray(got_saved) != saved)
        assert not len(bad), "%s: bits_saved of %r is %d, the oracle's %d" % (
            where, names[bad[0][0]][bad[0][1]], np.asarray(got_saved)[tuple(bad[0])], saved[tuple(bad[0])])
    bad = np.nonzero(np.asarray(got_offs) != offs)[0]
    assert not len(bad), "%s: block_offset[%d] is %d, expected %d" % (where, bad[0], np.asarray(got_offs)[bad[0]], offs[bad[0]])
    why = pc.first_difference(cfg, variant, got_bytes, want=image)
    assert why is None, what + ": " + why


def _forced(torch, cfg, n=None):
    return _dev(torch, pc.expected(cfg)["table"]["forced"][:n])


def _pack(torch, enc, cfg, inp, variant, n=None):
    """StreamEncoder.pack -> host arrays (bytes, block_offset, huff_table, bits_saved)"""
    got = enc.pack(cfg[3], cfg[4], inp, use_huffman=variant != "raw", huff_table=_forced(torch, cfg, n) if variant == "forced" else None)
    saved = None if got["bits_saved"] is None else got["bits_saved"].cpu().numpy()
    return got["bytes"].cpu().numpy(), got["block_offset"].cpu().numpy(), got["huff_table"].cpu().numpy(), saved


def _raw_pack(torch, hd, cfg, inp, variant, n, cap, m16):
    """Handle.dev_pack_blocks into a buffer of `cap` bytes with a canary behind it -> (total, buffer, offsets, table, saved)"""
    lay = pc.layout(cfg)
    buf = torch.full((cap + N_CANARY,), CANARY, dtype=torch.uint8, device="cuda:0")
    offs = torch.empty((n + 1,), dtype=torch.int64, device="cuda:0")
    table = torch.empty((n, lay["nch"]), dtype=torch.int32, device="cuda:0")
    saved = torch.empty((n, lay["nch"]), dtype=torch.int32, device="cuda:0")
    given = _forced(torch, cfg, n) if variant == "forced" else None
    sw = inp["ms_switch"].data_ptr() if lay["joint"] else None
    total = hd.dev_pack_blocks(cfg[3], cfg[4], n, lay["nch"], lay["joint"], variant != "raw", None if given is None else given.data_ptr(),
                               inp["overall_scale"].data_ptr(), sw, inp["scale_factor"].data_ptr(), inp["bit_alloc"].data_ptr(),
                               inp["mantissa"].data_ptr(), m16, buf.data_ptr(), cap, offs.data_ptr(), table.data_ptr(),
                               saved.data_ptr())
    return total, buf.cpu().numpy(), offs.cpu().numpy(), table.cpu().numpy(), (None if variant == "forced" else saved.cpu().numpy())


# ------------------------------------------------------------------------------------------------ pricers
@pytest.mark.parametrize("cfg", pc.CONFIGS, ids=IDS)
def test_huffman_gain_kernel_chooses_the_oracles_tables(torch, encoders, cfg):
    enc, lay, c, e = encoders[cfg[:3]], pc.layout(cfg), pc.cases(cfg), pc.expected(cfg)
    n, nch, names = len(c["names"]), lay["nch"], c["names"]
    ba, mant = c["bit_alloc"].reshape(n * nch, -1), c["mantissa"].reshape(n * nch, -1)
    want_t, want_s = e["table"]["priced"].reshape(-1), e["bits_saved"].reshape(-1)
    flat = [x for row in names for x in row]
    rng = np.random.default_rng(9)
    for ns in (1, 2):                                                   # waves per workgroup: one per stream
        m = (n * nch) // ns
        res = rng.integers(-1000, 100000, m).astype(np.int32)
        out = {"bit_alloc": _dev(torch, ba[:m * ns].reshape(m, ns, -1)), "mantissa": _dev(torch, mant[:m * ns].reshape(m, ns, -1)),
               "reservoir_out": _dev(torch, res)}
        table, saved, nxt = (t.cpu().numpy() for t in enc.huffman_gain(cfg[3], cfg[4], out))
        bad = np.nonzero(table.reshape(-1) != want_t[:m * ns])[0]
        assert not len(bad), "%s, %d streams: table of %r is %d, the oracle chooses %d" % (
            pc.config_id(cfg), ns, flat[bad[0]], table.reshape(-1)[bad[0]], want_t[bad[0]])
        bad = np.nonzero(saved.reshape(-1) != want_s[:m * ns])[0]
        assert not len(bad), "%s, %d streams: bits_saved of %r is %d, the oracle's %d" % (
            pc.config_id(cfg), ns, flat[bad[0]], saved.reshape(-1)[bad[0]], want_s[bad[0]])
        assert np.array_equal(nxt, res + want_s[:m * ns].reshape(m, ns).sum(axis=1))         # codecThem.py:224,274
        table, saved, nxt = (t.cpu().numpy() for t in enc.huffman_gain(cfg[3], cfg[4], out, use_huffman=False))
        assert (table == 15).all() and not saved.any() and np.array_equal(nxt, res)          # EncodeNoHuff


# ------------------------------------------------------------------------------------------------ plan + writer
@pytest.mark.parametrize("cfg", pc.CONFIGS, ids=IDS)
def test_device_packer_writes_the_oracles_bytes(torch, encoders, cfg):
    """all blocks in one call: priced on the device (pack_plan_kernel), raw, and with forced tables; int32 and 16-bit planes"""
    enc = encoders[cfg[:3]]
    for m16 in (False, True):
        inp = _inputs(torch, cfg, m16)
        for variant in pc.VARIANTS:
            _check(cfg, variant, *_pack(torch, enc, cfg, inp, variant), _want(cfg, variant), "all blocks, %s" % ("16-bit" if m16 else "int32"))


@pytest.mark.parametrize("cfg", pc.CONFIGS, ids=IDS)
def test_device_packer_on_small_batches(torch, encoders, cfg):
    """four waves share a workgroup: 1, 3, 4 and 5 blocks (1 to 10 chunks)"""
    enc = encoders[cfg[:3]]
    for m16 in (False, True):
        for n in (1, 3, 4, 5):
            inp = _inputs(torch, cfg, m16, index=slice(0, n))
            for variant in ("priced", "forced"):
                _check(cfg, variant, *_pack(torch, enc, cfg, inp, variant, n), _want(cfg, variant, n),
                       "%d blocks, %s" % (n, "16-bit" if m16 else "int32"))


@pytest.mark.parametrize("cfg", pc.CONFIGS, ids=IDS)
def test_device_packer_fills_a_buffer_of_exactly_the_total(torch, encoders, cfg):
    """out_cap == total: the call succeeds (the largest legal chunk, 22 bits on every line, stays within the writer's word
    image: no error 2), every byte is the oracle's and the 64 bytes behind the buffer are untouched"""
    enc = encoders[cfg[:3]]
    n = len(pc.cases(cfg)["names"])
    for m16, variant in ((False, "forced"), (True, "priced")):
        want = _want(cfg, variant)
        cap = int(want[1][-1])
        total, buf, offs, table, saved = _raw_pack(torch, enc.h, cfg, _inputs(torch, cfg, m16), variant, n, cap, m16)
        assert total == cap
        _check(cfg, variant, buf[:cap], offs, table, saved, want, "out_cap == total")
        assert (buf[cap:] == CANARY).all(), "%s: bytes behind out_cap written" % pc.config_id(cfg)


@pytest.mark.parametrize("cfg", LONG, ids=[pc.config_id(c) for c in LONG])
def test_generic_writer_at_1024_lines(torch, encoders, cfg):
    """a mantissa plane that starts 4 (int32) or 2 (16-bit) bytes past a 16-byte boundary: pack_fast16 declines, plan and
    writer take their generic paths with 16 lines per lane -- the same bytes"""
    enc = encoders[cfg[:3]]
    n = len(pc.cases(cfg)["names"])
    for m16 in (False, True):
        inp = _inputs(torch, cfg, m16, offset=True)
        for variant in ("priced", "forced"):
            want = _want(cfg, variant)
            cap = int(want[1][-1])
            total, buf, offs, table, saved = _raw_pack(torch, enc.h, cfg, inp, variant, n, cap, m16)
            assert total == cap
            _check(cfg, variant, buf[:cap], offs, table, saved, want, "offset plane, %s" % ("16-bit" if m16 else "int32"))
            assert (buf[cap:] == CANARY).all()


# ------------------------------------------------------------------------------------------------ position scan
@pytest.mark.parametrize("mode", ["mono", "joint"])
def test_long_batches_cross_the_scan_tiles(torch, encoders, mode):
    lb = pc.long_batch(mode)
    cfg = lb["cfg"]
    names = [pc.cases(cfg)["names"][i] for i in lb["index"]]
    got = encoders[cfg[:3]].pack(cfg[3], cfg[4], _inputs(torch, cfg, index=lb["index"]))
    assert np.array_equal(got["huff_table"].cpu().numpy(), lb["table"]) and np.array_equal(got["bits_saved"].cpu().numpy(), lb["bits_saved"])
    offs = got["block_offset"].cpu().numpy()
    bad = np.nonzero(offs != lb["offsets"])[0]
    assert not len(bad), "block_offset[%d] is %d, expected %d" % (bad[0], offs[bad[0]], lb["offsets"][bad[0]])
    assert got["bytes"].numel() == lb["image"].size                        # the total
    why = pc.first_difference(cfg, "priced", got["bytes"].cpu().numpy(), names=names, offsets=lb["offsets"], want=lb["image"])
    assert why is None, why


# ------------------------------------------------------------------------------------------------ parser
def _dev_parse(torch, hd, image, chunk_offsets, nch, joint):
    n = len(chunk_offsets) // nch
    buf, offs = _dev(torch, image), _dev(torch, chunk_offsets)
    shapes = dict(a=(n,), b=(n,), huff_table=(n, nch), overall_scale=(n, 4 if joint else nch), ms_switch=(n, 32),
                  scale_factor=(n, nch, 32), bit_alloc=(n, nch, 32), mantissa=(n, nch, hd.cfg.n_mdct_lines))
    out = {k: torch.zeros(s, dtype=torch.int32, device="cuda:0") for k, s in shapes.items()}
    p = lambda k: out[k].data_ptr()
    hd.dev_unpack_blocks(n, nch, joint, buf.data_ptr(), buf.numel(), offs.data_ptr(), p("a"), p("b"), p("huff_table"),
                         p("overall_scale"), p("ms_switch"), p("scale_factor"), p("bit_alloc"), p("mantissa"))
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("cfg", pc.CONFIGS, ids=IDS)
def test_device_parser_returns_the_crafted_integers(torch, encoders, cfg):
    lay, e = pc.layout(cfg), pc.expected(cfg)
    for variant in ("forced", "raw"):
        got = _dev_parse(torch, encoders[cfg[:3]].h, e["image"][variant], pc.chunk_offsets(cfg, variant), lay["nch"], lay["joint"])
        why = pc.parsed_difference(cfg, variant, got)
        assert why is None, why


def test_device_parser_on_the_joint_long_batch(torch, encoders):
    lb = pc.long_batch("joint")
    cfg = lb["cfg"]
    got = _dev_parse(torch, encoders[cfg[:3]].h, lb["image"], lb["chunk_offsets"], 2, True)
    want = {k: (None if v is None else v[lb["index"]]) for k, v in pc.parsed(cfg, "priced").items()}
    why = pc.parsed_difference(cfg, "priced", got, want=want, names=[pc.cases(cfg)["names"][i] for i in lb["index"]])
    assert why is None, why
