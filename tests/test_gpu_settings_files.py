"""
GPU tests of the file-level paths at the codec settings of tests/settings_kit.py (block lengths 512/256, 256/128, 1024/512
and 768/384, other scale-factor / allocation-field / block-switch field widths, the reference's training settings): the
chained stereo and mono encodes and the rate ladder against the oracle's writer byte for byte; the device packer and the
device chunk parser against the host packer and the host parser; the whole-file decodes against oracle.decode.decode_pac;
the resident store against slices of those decodes; mrc_pac_nmr against its restatement; the constant-quality VBR and
target-NMR encodes against theirs; and files without block-switch fields.  Every bar is byte or integer equality, or the
bar of the default-setting test named beside it.  One handle per setting for the module.
"""
import re

import numpy as np
import pytest

import chain_kit as kit
import settings_kit as SK
import test_gpu_device_decode as DD
import test_gpu_devpack as DP
import unpack_corpus as UC
from oracle import decode as odec, pacfile as opac

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LADDER = {"B": (2.0, 4.0), "E": (1.5, 3.0), "F": (2.0, 3.5), "H": (1.5, 2.86)}


@pytest.fixture(scope="module")
def handles():
    from mrcaudiocodec_amd import Handle
    made = {}

    def get(sid):
        if sid not in made:
            made[sid] = Handle(device_id=0, **SK.handle_kwargs(sid))
        return made[sid]
    try:
        yield get
    finally:
        for hd in made.values():
            hd.close()


def test_lengths_that_do_not_factor_are_refused():
    from mrcaudiocodec_amd import Handle, MrcError
    for L, S in SK.REFUSED_LENGTHS:
        with pytest.raises(MrcError, match="factor into 2s and 3s"):
            Handle(device_id=0, n_mdct_lines=L, n_short=S)


# ------------------------------------------------------------------ 1, 2, 3: the chained encodes
@pytest.mark.parametrize("huff", [True, False])
@pytest.mark.parametrize("sid", SK.IDS)
def test_stereo_chained_encode_equals_the_oracle(handles, sid, huff):
    from mrcaudiocodec_amd import pacfile as ppac
    h, pcm = handles(sid), SK.stream(sid)
    want = [SK.oracle_file(sid, 2, huff, which)["data"] for which in (0, 1)]
    assert ppac.encode_stereo_stream(h, pcm, SK.schedule(sid), use_huffman=huff) == want[0]
    assert ppac.encode_stereo_stream_per_block(h, SK.to_float(pcm), SK.schedule(sid), use_huffman=huff) == want[0]
    both = ppac.encode_stereo_streams(h, np.stack([pcm, pcm]), [SK.schedule(sid, 0), SK.schedule(sid, 1)], use_huffman=huff)
    assert both == want
    assert ppac.encode_stereo_stream(h, SK.to_float(pcm), SK.schedule(sid, 1), use_huffman=huff) == want[1]      # float input


@pytest.mark.parametrize("huff", [True, False])
@pytest.mark.parametrize("sid", SK.IDS)
def test_mono_chained_encode_equals_the_oracle(handles, sid, huff):
    from mrcaudiocodec_amd import pacfile as ppac
    h, pcm = handles(sid), SK.mono(sid)
    want = SK.oracle_file(sid, 1, huff)["data"]
    assert ppac.encode_mono_stream(h, pcm[0], SK.schedule(sid), use_huffman=huff) == want
    assert ppac.encode_mono_stream_per_block(h, SK.to_float(pcm[0]), SK.schedule(sid), use_huffman=huff) == want
    two = ppac.encode_mono_streams(h, np.stack([pcm[0], pcm[0]]), [SK.schedule(sid, 1), SK.schedule(sid, 0)], use_huffman=huff)
    assert two == [SK.oracle_file(sid, 1, huff, 1)["data"], want]


@pytest.mark.parametrize("nch", [2, 1])
@pytest.mark.parametrize("sid", sorted(LADDER))
def test_ladder_equals_the_oracle_at_each_rate(handles, sid, nch):
    from mrcaudiocodec_amd import pacfile as ppac
    h = handles(sid)
    got = ppac.encode_stream_ladder(h, SK.stream(sid)[:nch], SK.schedule(sid), LADDER[sid])
    want = [SK.oracle_file(sid, nch, True, bits_per_sample=r)["data"] for r in LADDER[sid]]
    assert got == want and want[0] != want[1]


# ------------------------------------------------------------------ 4: device packer and device parser
def _dev(arr, dtype=torch.int32):
    return torch.as_tensor(np.ascontiguousarray(arr), device="cuda:0").to(dtype).contiguous()


@pytest.mark.parametrize("sid", SK.IDS)
def test_device_packer_equals_the_host_packer(handles, sid):
    """test_gpu_devpack._check on the setting's encoder output (blocks of the kit's stream, every shape, independent and
    joint, both mantissa formats; priced, raw, tables given) and on hand-built blocks with allocations up to maxMantBits"""
    from mrcaudiocodec_amd import pacfile as ppac
    from mrcaudiocodec_amd.batch import StreamEncoder
    h, cfg = handles(sid), SK.config(sid)
    enc = StreamEncoder(handle=h)
    x = SK.to_float(SK.stream(sid))
    left, right = _dev(x[0], torch.float64), _dev(x[1], torch.float64)
    L, S = SK.lengths(sid)
    rng = np.random.default_rng(ord(sid))
    for (a, b) in SK.shapes_of(sid):
        at = np.linspace(0, x.shape[1] - (a + b), 24).astype(np.int64)     # 24 blocks over the loud and the quiet half
        n = len(at)
        assert at[-1] + a + b == x.shape[1] and len(set(at.tolist())) == n
        offs = _dev(at, torch.int64)
        res = _dev(rng.integers(0, 200, n))
        for joint in (False, True):
            for m16 in (False, True):
                out = dict(enc.encode(a, b, left, right if joint else None, n, 0, offs, res, mantissa16=m16))
                got = DP._check(torch, ppac, enc, cfg, a, b, joint, out, True)
                DP._check(torch, ppac, enc, cfg, a, b, joint, out, False)
                DP._check(torch, ppac, enc, cfg, a, b, joint, out, True, given=got["huff_table"].contiguous())
            osc, sw, sf, ba, mant = UC._random_blocks(cfg, a, b, 24, 2, rng)
            assert ba.max() == SK.max_mant_bits(sid)
            nch = 2 if joint else 1
            crafted = {"overall_scale": _dev(osc if joint else osc[:, :1]), "scale_factor": _dev(sf[:, :nch]),
                       "bit_alloc": _dev(ba[:, :nch]), "mantissa": _dev(mant[:, :nch])}
            if joint:
                crafted["ms_switch"] = _dev(sw)
            for use_huffman in (True, False):
                DP._check(torch, ppac, enc, cfg, a, b, joint, crafted, use_huffman)
            forced = _dev(rng.choice([0, 1, 2, 3, 15], (24, nch)))
            DP._check(torch, ppac, enc, cfg, a, b, joint, crafted, True, given=forced)


@pytest.mark.parametrize("sid", SK.IDS)
def test_device_parser_equals_the_host_parser(handles, sid):
    """test_gpu_device_decode._compare on the oracle's files of the setting, on chunks with every table forced, and on 300
    seeded corruptions of them: the same accept / reject decisions, the same integers"""
    h = handles(sid)
    cases = SK.file_cases(sid) + SK.forced_table_cases(sid)
    n_acc, n_rej = DD._compare(cases, h)
    assert n_rej == 0 and n_acc == len(cases)
    n_acc, n_rej = DD._compare(UC.corruptions(cases, n=300, seed=100 + ord(sid)), h)
    assert n_acc > 0 and n_rej > 0 and n_acc + n_rej == 300
    assert DD._compare(cases[:2], h) == (2, 0)                              # still well after the refusals


# ------------------------------------------------------------------ 5: whole-file decode
def _files(sid):
    """the setting's files: stereo (Huffman, raw), mono, one-block stereo, one-block mono, a header alone"""
    from mrcaudiocodec_amd import pacfile as ppac
    cfg = SK.config(sid)
    stereo, raw, mono = (SK.oracle_file(sid, 2, True)["data"], SK.oracle_file(sid, 2, False)["data"],
                         SK.oracle_file(sid, 1, True)["data"])
    head2, head1 = len(ppac.header(cfg, 2, 0)), len(ppac.header(cfg, 1, 0))
    last2 = int(ppac.index(stereo, cfg)["chunk_offset"][-1, 0])
    last1 = int(ppac.index(mono, cfg)["chunk_offset"][-1, 0])
    return [stereo, raw, mono, stereo[:head2] + stereo[last2:], mono[:head1] + mono[last1:], stereo[:head2]]


@pytest.fixture(scope="module")
def decoded(handles):
    """per setting: the files, the library's float64 planes and 16-bit codes of them (computed once, read-only)"""
    from mrcaudiocodec_amd import pacfile as ppac
    made = {}

    def get(sid):
        if sid not in made:
            h, L = handles(sid), SK.lengths(sid)[0]
            files = _files(sid)
            f64 = [ppac.decode_pac(h, f)[1].cpu().numpy() for f in files[:-1]]
            pcm = ppac.decode_pac_files(h, files)
            for a in f64 + list(pcm):
                a.setflags(write=False)
            made[sid] = dict(files=files, f64=f64, pcm=[np.ascontiguousarray(p) for p in pcm], L=L)
        return made[sid]
    return get


@pytest.mark.parametrize("sid", SK.IDS)
def test_whole_file_decode_equals_the_oracle(handles, decoded, sid):
    from mrcaudiocodec_amd import pacfile as ppac
    h, d = handles(sid), decoded(sid)
    files, L = d["files"], d["L"]
    inter = h.decode_pac_pcm16(files)                                        # WAV order
    assert len(inter) == len(files) == 6
    for i, f in enumerate(files[:-1]):
        want = SK.oracle_decode(sid, f)
        got = d["f64"][i]
        assert got.shape == want.shape
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), (i, np.max(np.abs(got - want)) / np.max(np.abs(want)))
        codes = odec.pcm16(want[:, L:])
        assert np.array_equal(ppac.decode_pac_pcm16(h, f), codes), i
        assert d["pcm"][i].dtype == np.int16 and np.array_equal(d["pcm"][i], codes), i
        assert np.array_equal(inter[i].T, codes), i
    assert [p.shape[0] for p in d["pcm"]] == [2, 2, 1, 2, 1, 2]
    assert d["pcm"][3].shape[1] == d["pcm"][4].shape[1] == L                 # one block: its b samples
    assert d["pcm"][5].shape == (2, 0) and inter[5].shape == (0, 2)          # the header alone
    assert SK.oracle_decode(sid, files[5]).shape[1] == 0 or not SK.oracle_decode(sid, files[5]).any()


# ------------------------------------------------------------------ 6: the resident store
def _needed(ix, start, window, L):
    """the overlap rule of the store with the setting's L: blocks with block_start < start + window + L and
    block_start + a + b > start + L"""
    p = ix["block_start"]
    return int(np.count_nonzero((p < start + window + L) & (p + ix["block_a"] + ix["block_b"] > start + L)))


@pytest.mark.parametrize("sid", [s for s in SK.IDS if 6 in SK.COVERS[s]])
def test_store_windows_equal_the_whole_file_decodes(handles, decoded, sid):
    from mrcaudiocodec_amd import pacfile as ppac
    from mrcaudiocodec_amd.store import PacStore
    from test_gpu_store import _cut
    h, d = handles(sid), decoded(sid)
    L, S = SK.lengths(sid)
    files, pcm = d["files"], d["pcm"]
    f64 = [np.ascontiguousarray(x[:, L:]) for x in d["f64"]] + [np.zeros((2, 0))]
    index = [ppac.index(f, SK.config(sid)) for f in files]
    with PacStore(h, files) as store:
        assert store.n_samples.tolist() == [p.shape[1] for p in pcm] and store.n_channels.tolist() == [2, 2, 1, 2, 1, 2]
        for f in (0, 2, 3, 4, 5):
            n = pcm[f].shape[1]
            wins = [(w, s) for w in (1, S, L, 3 * L + 5, n + 2 * L) for s in (0, -1, n - 1, -w, n)]     # both file ends
            for p in index[f]["block_start"].tolist():                       # every block boundary, in sample positions
                wins += [(11, p - L - 5), (S + 3, p - L - S // 2)]
            for w, s in wins:
                one = store.decode_window([f], [s], w)
                assert one.dtype == torch.int16 and tuple(one.shape) == (1, pcm[f].shape[0], w)
                assert np.array_equal(one[0].cpu().numpy(), _cut(pcm[f], s, w)), (f, w, s)
                st = store.stats()
                assert st["chunks_parsed"] == _needed(index[f], s, w, L) * index[f]["n_channels"], (f, w, s)
                x = store.decode_window([f], [s], w, dtype=torch.float64)[0].cpu().numpy()
                ref = _cut(f64[f], s, w)
                assert np.array_equal(x, ref) and np.array_equal(np.signbit(x), np.signbit(ref)), (f, w, s)
                x32 = store.decode_window([f], [s], w, dtype=torch.float32)[0].cpu().numpy()
                assert np.array_equal(x32, ref.astype(np.float32)), (f, w, s)
        # many windows of several files in one call
        items = [(f, s) for f in range(len(files)) for s in range(-L - 7, pcm[f].shape[1] + L, L // 2 + 29)]
        fs, ss = zip(*items)
        got = store.decode_window(fs, ss, S + 44).cpu().numpy()
        for k, (f, s) in enumerate(items):
            assert np.array_equal(got[k], np.broadcast_to(_cut(pcm[f], s, S + 44), got[k].shape)), (f, s)   # (mono: both rows)


# ------------------------------------------------------------------ 7: the noise-to-mask ratio
@pytest.mark.parametrize("nch", [2, 1])
@pytest.mark.parametrize("sid", SK.IDS)
def test_nmr_equals_the_restatement(handles, sid, nch):
    from mrcaudiocodec_amd import pacfile as ppac
    h = handles(sid)
    buf, src = SK.oracle_file(sid, nch, True)["data"], SK.source(sid, nch)
    got = h.pac_nmr(buf, src, detail=True)[0]
    want = kit.check_nmr_against_restatement(got, buf, src, SK.lengths(sid)[1], SK.blksw(sid))
    kit.check_nmr_summaries(got)
    assert {tuple(s) for s in got["shape"]} == set(SK.shapes_of(sid))
    brief = ppac.measure_nmr(h, buf, src)
    assert brief["n_blocks"] == want["n_blocks"] == len(SK.schedule(sid)) + 1
    assert brief["nmr_max_db"] == got["nmr_max_db"] and brief["nmr_total_db"] == got["nmr_total_db"]


# ------------------------------------------------------------------ 8: constant-quality VBR and target-NMR
VBR_CEILINGS = (6.0, -12.0)        # chosen on the CPU: the restatement meets no edge candidate at B, C, F, H (asserted below)
VBR_SETTINGS = [s for s in SK.IDS if 8 in SK.COVERS[s]]


@pytest.mark.parametrize("nch", [2, 1])
@pytest.mark.parametrize("sid", VBR_SETTINGS)
def test_vbr_nmr_equals_the_restatement(handles, sid, nch):
    """the checks of test_gpu_vbr._check, and one encode_stream_vbr_size call against the vbr_nmr file of its ceiling"""
    import vbr_restatement as vr
    from mrcaudiocodec_amd import pacfile as ppac
    h, pcm, sch = handles(sid), SK.stream(sid)[:nch], SK.schedule(sid)
    files = []
    for db in VBR_CEILINGS:
        g = ppac.encode_stream_vbr_nmr(h, pcm, sch, db)
        assert g["ceiling_ratio"] == vr.ceiling_ratio(db)
        w = vr.encode(pcm, sch, g["ceiling_ratio"], cp=SK.coding_params(sid, nch))
        assert w["edges"] == 0, "the input was chosen to have no edge candidate"
        assert g["data"] == w["data"], (db, len(g["data"]), len(w["data"]))
        assert g["capped_bands"] == w["capped"] and g["coded_bits"] == vr.coded_bits(w["data"], nch)
        assert g["n_blocks"] == len(sch) + 1
        files.append(g["data"])
    assert len(files[0]) < len(files[1])                                    # the tighter ceiling costs bytes
    if sid in "FH":
        assert w["capped"] > 0                                              # few mantissa bits: bands that never meet it
    lo, step, n = VBR_CEILINGS[1], 6.0, 4                                   # the grid -12, -6, 0, 6 dB
    target = (len(files[0]) + len(files[1])) // 2
    r = ppac.encode_stream_vbr_size(h, pcm, sch, target, lo_db=lo, step_db=step, n=n)
    sizes = [len(ppac.encode_stream_vbr_nmr(h, pcm, sch, float(db))["data"]) for db in ppac.ceiling_grid(lo, step, n)]
    chosen, met, probed = ppac.bisect_ceiling(sizes, target)
    assert (r["chosen"], r["met"]) == (chosen, met) and met and r["chosen_db"] == ppac.ceiling_grid(lo, step, n)[chosen]
    assert r["data"] == ppac.encode_stream_vbr_nmr(h, pcm, sch, r["chosen_db"])["data"] and len(r["data"]) <= target


@pytest.mark.parametrize("nch", [2, 1])
@pytest.mark.parametrize("sid", VBR_SETTINGS)
def test_target_nmr_on_a_two_rung_ladder(handles, sid, nch):
    """the checks of test_gpu_target_nmr._check with the oracle's files as the rungs: per rung the numbers of mrc_pac_nmr for
    the oracle's file at that rate, the rung by pacfile.choose_rung, its bytes the oracle's"""
    import nmr_restatement as nr
    from mrcaudiocodec_amd import pacfile as ppac
    h, pcm, sch = handles(sid), SK.stream(sid)[:nch], SK.schedule(sid)
    rates = LADDER[sid] if sid in LADDER else (2.0, 4.0)
    files = [SK.oracle_file(sid, nch, True, bits_per_sample=r)["data"] for r in rates]
    src = SK.source(sid, nch)
    measured = ppac.measure_nmr(h, files, src)
    restated = [nr.restate(f, src, SK.lengths(sid)[1], SK.blksw(sid))["nmr_total_db"] for f in files]
    assert restated[1] < restated[0] - 0.2                                  # the targets below lie 0.1 dB or more from a rung
    for target in (0.5 * (restated[0] + restated[1]), restated[0] + 1.0, restated[1] - 1.0):
        g = ppac.encode_stream_target_nmr(h, pcm, sch, rates, target)
        for k, w in enumerate(measured):
            assert g["nmr_total_db"][k] == w["nmr_total_db"] and g["nmr_max_db"][k] == w["nmr_max_db"]
            assert g["disturbed_blocks"][k] == w["disturbed_blocks"] and g["n_blocks"] == w["n_blocks"]
        chosen, met = ppac.choose_rung(restated, target)
        assert (g["chosen"], g["met"], g["rate"]) == (chosen, met, rates[chosen])
        assert g["data"] == files[chosen]


# ------------------------------------------------------------------ 9: no block-switch fields
def test_short_blocks_without_switch_fields(handles):
    """Block-switch width 0: a schedule with short blocks encodes to the oracle's bytes, but nothing in a chunk says that it
    is short.  Every decoder reads it as a long block, runs out of payload in the first short block and refuses the file;
    the host parser and the device paths name the same chunk with the same words, and the handle works afterwards."""
    from mrcaudiocodec_amd import MrcError, pacfile as ppac
    from mrcaudiocodec_amd.store import PacStore
    sid = "J"
    h, cfg = handles(sid), SK.config(sid)
    L, S = SK.lengths(sid)
    sch = SK._chain([(L, L), (L, S)] + [(S, S)] * (L // S - 1) + [(S, L), (L, L)])
    pcm = SK.stream(sid)
    texts = {}
    for nch in (2, 1):
        x = SK.to_float(pcm[:nch])
        if nch == 2:
            want = opac.encode_stereo_stream(x, sch, cp=SK.coding_params(sid, 2), huffman=True)
            assert ppac.encode_stereo_stream(h, pcm, sch) == want
        else:
            import mono_oracle
            want = mono_oracle.encode_mono_stream(x, sch, cp=SK.coding_params(sid, 1), huffman=True)
            assert ppac.encode_mono_stream(h, pcm[0], sch) == want
        # the host parser: block by block, the first it refuses
        cases = UC._file_cases(want, "short", cfg)
        first = cases[0]
        assert UC.host_parse(first) is None
        offs = np.asarray(first["offsets"]).reshape(-1, nch)
        bad = [i for i in range(len(offs)) if UC.host_parse(dict(first, offsets=offs[i])) is None]
        assert bad and bad[0] >= 1                                         # (the first block is long)
        with pytest.raises(MrcError) as e0:
            ppac.decode_pac(h, want)                                       # the host parser's path
        src = np.ascontiguousarray(pcm[:nch, L:sch[-1][0] + 2 * L])
        with pytest.raises(MrcError) as e1:
            ppac.decode_pac_files(h, [want])
        with pytest.raises(MrcError) as e2:
            h.pac_nmr(want, src)
        with PacStore(h, [want]) as store:
            with pytest.raises(MrcError) as e3:
                store.decode_window([0], [0], int(store.n_samples[0]))
        tails = []
        for e in (e0, e1, e2, e3):
            assert e is e0 or e.value.code == -1
            m = re.search(r"chunk at byte (\d+): (.*)$", str(e.value))
            assert m, str(e.value)
            tails.append((int(m.group(1)), m.group(2)))
        assert tails[0] == tails[1] == tails[2] == tails[3], tails             # host and device: one chunk, one text
        assert all("file 0: " in str(e.value) for e in (e1, e2, e3))
        assert tails[0][0] in offs[bad[0]].tolist(), (tails, offs[bad[0]])    # the first block the host parser refuses
        texts[nch] = tails[0][1]
    assert texts[1] == texts[2]
    # the handle still works: the long-only file of the setting
    good = SK.oracle_file(sid, 2, True)["data"]
    assert ppac.encode_stereo_stream(h, pcm, SK.schedule(sid)) == good
    assert np.array_equal(ppac.decode_pac_files(h, [good])[0], odec.pcm16(SK.oracle_decode(sid, good)[:, L:]))
