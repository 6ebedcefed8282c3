"""
CPU side of the crafted decode cases (tests/decode_cases.py): the oracle alone and the host code, no GPU.  It holds the INPUT to
what tests/test_gpu_decode_cases.py relies on: the families are what they claim, the files round-trip through the oracle's
own reader and through the library's host parser, no oracle sample sits on a 16-bit code boundary (so the GPU file may compare
PCM codes exactly), and -- the evidence of what the crafted files add -- a restatement of the oracle's line decoder with one
plausible slip at a time differs from the oracle, on a crafted file, by more than the bar the GPU file applies.

The mutant table (printed by test_mutants_are_exposed, kept in DESIGN.md section 2) says per slip which crafted files expose it
and whether the encoder-made kit files (settings_kit.oracle_file, mix_restatement.files) do.
"""
import numpy as np
import pytest

import decode_cases as dc
import mix_restatement as MR
import reduced_restatement as RR
import settings_kit as SK
from oracle import decode as odec

BAR = 1e-12                       # of the file's peak: the bar of every path of tests/test_gpu_decode_cases.py (b) to (f)
MUTATIONS = {                     # name -> the path whose planes it changes
    "half_step_on_zero_codes": "lines", "half_step_at_cap": "lines", "sign_threshold_one_bit_off": "lines", "cap_always_15": "lines",
    "ms_scales_exchanged": "lines", "lr_scales_in_ms_bands": "lines", "switch_ignored_where_a_stream_has_no_bits": "lines",
    "side_sign_flipped": "lines", "mid_without_the_half": "mid", "reduced_reads_one_line_more": "reduced",
}


# ------------------------------------------------------------------------------------------------ a: the families
@pytest.mark.parametrize("sid", dc.SETTINGS)
def test_families_are_what_they_claim(sid):
    f = dc.settings(sid)
    cap, top = f["cap"], f["top"]
    for (a, b) in dc.shapes_of(sid):
        lay = dc.layout(sid, a, b)
        nb, half, band_of = lay["nb"], lay["half"], lay["band_of"]
        for fam in dc.families(sid):
            for joint in (False, True):
                if not joint and fam in dc.JOINT_ONLY:
                    continue
                blks = dc.blocks(sid, fam, a, b, joint)
                assert blks, (fam, a, b, joint)
                for blk in blks:
                    assert blk["family"] == fam and len(blk["ba"]) == (2 if joint else 1) and len(blk["os"]) == (4 if joint else 1)
                    assert all(0 <= s <= cap for s in blk["os"])
                    for sf, ba, m in zip(blk["sf"], blk["ba"], blk["mant"]):
                        bits = ba.astype(np.int64)[band_of]
                        assert ba.shape == (nb,) and m.shape == (half,) and sf.min() >= 0 and sf.max() <= cap
                        assert not (ba == 1).any() and ba.min() >= 0 and ba.max() <= top
                        assert (m[bits == 0] == 0).all() and (m >= 0).all() and (m < (1 << bits)).all()
        # full: the widest allocation in every band, every magnitude at its maximum, signs alternating, both overall scales
        full = dc.blocks(sid, "full", a, b, True) + dc.blocks(sid, "full", a, b, False)
        for blk in full:
            for sf, ba, m in zip(blk["sf"], blk["ba"], blk["mant"]):
                assert (ba == top).all() and (sf == cap).all() and ((m & ((1 << (top - 1)) - 1)) == (1 << (top - 1)) - 1).all()
                assert ((m >> (top - 1))[1:] != (m >> (top - 1))[:-1]).all()
        assert {tuple(blk["os"]) for blk in full} == {(0,), (cap,), (0,) * 4, (cap,) * 4}
        # switch: every pattern; every combination of (switch, which stream has bits); the scales in two orders
        sw = {blk["name"].split("/")[1]: blk for blk in dc.blocks(sid, "switch", a, b, True)}
        assert set(sw) == set(dc.SWITCH_PATTERNS)
        j = np.arange(nb)
        assert not sw["all0"]["ms"].any() and sw["all1"]["ms"].all() and np.array_equal(sw["alternating"]["ms"], j % 2)
        assert np.array_equal(sw["first_only"]["ms"], j == 0) and np.array_equal(sw["last_only"]["ms"], j == nb - 1)
        for name in ("occupancy0", "occupancy1"):
            blk = sw[name]
            combos = {(int(blk["ms"][q]), bool(blk["ba"][0][q]), bool(blk["ba"][1][q])) for q in range(nb)}
            assert len(combos) == 8, (sid, a, b, name, combos)
        s0, s1 = sw["scales0"]["os"], sw["scales1"]["os"]
        assert s0 != s1 and {0, cap} <= set(s0) and {0, cap} <= set(s1) and sw["scales0"]["ms"].any() and not sw["scales0"]["ms"].all()
        assert (len(set(s0)) == 4 and sorted(s0) == sorted(s1)) if cap >= 3 else (s0[0] != s0[2] and s0[1] != s0[3] and s0[2] != s0[3])
        if sid not in dc.FULL_SETS:
            continue
        # sign_only: the sign bit alone at 2, 3 and the widest allocation
        so = dc.blocks(sid, "sign_only", a, b, False)
        assert {int(blk["ba"][0][0]) for blk in so} == {2, min(3, top), top}
        assert all((blk["mant"][0] == 1 << (int(blk["ba"][0][0]) - 1)).all() for blk in so)
        # ladder: scale factor j mod (cap + 1) up to a rotation, allocations cycling 2..top, magnitudes max / 1 / 0 in turn
        ladder = dc.blocks(sid, "ladder", a, b, False)
        assert {0, cap} <= set(np.concatenate([blk["sf"][0] for blk in ladder]).tolist())     # (9 bands: over the two variants)
        assert {2, top} <= set(np.concatenate([blk["ba"][0] for blk in ladder]).tolist())
        for blk in ladder:
            sf, ba, m = blk["sf"][0], blk["ba"][0].astype(np.int64), blk["mant"][0].astype(np.int64)
            assert ((np.diff(sf) % (cap + 1)) == 1).all() and ((np.diff(ba) == 1) | (np.diff(ba) == 2 - top)).all() and ba.min() >= 2
            bits = ba[band_of]
            mag = m & ((1 << (bits - 1)) - 1)
            assert {0, 1} <= set(mag.tolist()) and (mag[(mag != 0) & (mag != 1)] == ((1 << (bits - 1)) - 1)[(mag != 0) & (mag != 1)]).all()
            assert ((m >> (bits - 1)) == 1).any() and ((m >> (bits - 1)) == 0).any()
        # one_line: one non-zero code, on every position -- the lines either side of the reduced cuts among them
        pos = dc.one_line_positions(sid, a, b)
        assert pos["cut2_below"] == half // 2 - 1 and pos["cut2_at"] == half // 2 and pos["cut4_below"] == half // 4 - 1 and pos["cut4_at"] == half // 4
        assert pos["first"] == 0 and pos["last"] == half - 1 and band_of[pos["band_lo"]] == band_of[pos["band_hi"]]
        assert band_of[pos["band_lo"] - 1] != band_of[pos["band_lo"]] and band_of[pos["band_hi"] + 1] != band_of[pos["band_hi"]]
        for joint in (False, True):
            seen = set()
            for blk in dc.blocks(sid, "one_line", a, b, joint):
                m = np.concatenate(blk["mant"])
                assert np.count_nonzero(m) == 1 and sum(int((ba > 0).sum()) for ba in blk["ba"]) == 1
                _, p, t = blk["name"].split("/")
                line = int(np.flatnonzero(m)[0]) % half
                assert line == pos[p] and int(m.max()) == dc.one_line_triples(sid)[int(t)][2]
                seen.add((p, int(t), int(np.flatnonzero(m)[0]) // half))
            assert {(p, t) for p, t, _ in seen} == {(p, t) for p in dc.ONE_LINE_POSITIONS for t in (0, 1)}
            assert not joint or {s for _, _, s in seen} == {0, 1}                   # the line in either stream
        for blk in dc.blocks(sid, "idle_fields", a, b, True):
            assert not any(ba.any() for ba in blk["ba"]) and all(sf.all() for sf in blk["sf"]) and all(blk["os"])


@pytest.mark.parametrize("sid", dc.SETTINGS)
def test_files_chain_and_hold_every_family_in_every_shape(sid):
    f = dc.settings(sid)
    L = f["L"]
    for pf in dc.files(sid):
        blks = pf["blocks"]
        assert all(x["b"] == y["a"] for x, y in zip(blks[:-1], blks[1:])) and blks[0]["a"] == L and blks[-1]["b"] == L
        assert {(x["a"], x["b"]) for x in blks} == set(dc.shapes_of(sid)) and (len(dc.shapes_of(sid)) == 4 or sid == "J")
        fams = [fam for fam in dc.PARTS[pf["part"]] if fam in dc.families(sid) and (pf["n_channels"] == 2 or fam not in dc.JOINT_ONLY)]
        assert {(x["family"], x["a"], x["b"]) for x in blks} == {(fam, a, b) for fam in fams for (a, b) in dc.shapes_of(sid)}
        assert all(x["joint"] for x in blks[:-1]) == (pf["n_channels"] == 2) and not blks[-1]["joint"]
        if pf["n_channels"] == 2:
            ms = np.concatenate([x["ms"] for x in blks if x["joint"]])
            assert (ms == 1).any() and (ms == 0).any()                                  # both kinds of band
            assert blks[-1]["nch"] == 2 and blks[-1]["os"][0] != blks[-1]["os"][1]     # Close()'s pair: two scales
        if pf["part"] == "one_line":                                                   # one pass per line position
            names = {x["name"].split("/")[1] for x in blks[:-1] if x["family"] == "one_line"}
            assert names == set(dc.ONE_LINE_POSITIONS)
        if pf["huffman"]:
            tabs = {t for row in pf["tables"] for t in row}
            if pf["part"] == "full":                                                   # every code at its maximum: no table wins
                assert tabs == {15} and pf["data"] == dc.pac_file(sid, pf["n_channels"], False, "full")["data"]
            else:                                                                      # chunks on tables (main: raw ones too)
                assert tabs - {15} and 15 in tabs
                assert pf["data"] != dc.pac_file(sid, pf["n_channels"], False, pf["part"])["data"]
        x = dc.planes(sid, pf["n_channels"], pf["part"])
        assert x.shape == (pf["n_channels"], int(pf["block_start"][-1]) + 2 * L)
    if sid in dc.HUFFMAN_SETS:                                                         # three of the four tables over the images
        assert len({t for pf in dc.files(sid) for row in pf["tables"] for t in row} - {15}) >= 3


# ------------------------------------------------------------------------------------------------ b, c: the readers
def _parsed(pf):
    """the oracle's own reader on the file -> [dict per block], once per file (parse_any below)"""
    f = dc.settings(pf["sid"])
    return [p for p, _, _ in _parse_once(pf["label"], pf["data"], f["S"], f["blksw"])[1]]


def _same_integers(got, blk, who):
    assert (got["a"], got["b"]) == (blk["a"], blk["b"]), who
    assert [int(v) for v in got["os"]] == [int(v) for v in blk["os"]], who
    if blk["joint"]:
        assert np.array_equal(np.asarray(got["ms"])[:len(blk["ms"])], blk["ms"]), who
    for c in range(len(blk["ba"])):
        nb, half = len(blk["ba"][c]), len(blk["mant"][c])
        assert np.array_equal(np.asarray(got["sf"][c])[:nb], blk["sf"][c]), who
        assert np.array_equal(np.asarray(got["ba"][c])[:nb], blk["ba"][c]), who
        assert np.array_equal(np.asarray(got["mant"][c])[:half], blk["mant"][c]), who


@pytest.mark.parametrize("sid", dc.SETTINGS)
def test_oracle_reader_returns_the_crafted_integers(sid):
    for pf in dc.files(sid):
        got = _parsed(pf)
        assert len(got) == len(pf["blocks"])
        for i, (g, blk) in enumerate(zip(got, pf["blocks"])):
            _same_integers(g, blk, (sid, pf["n_channels"], pf["huffman"], i, blk["name"]))
            assert list(g["table"]) == list(pf["tables"][i])


@pytest.mark.parametrize("sid", dc.SETTINGS)
def test_host_parser_returns_the_crafted_integers(sid):
    from mrcaudiocodec_amd import pacfile as ppac
    cfg = dc.config(sid)
    for pf in dc.files(sid):
        nch, blks = pf["n_channels"], pf["blocks"]
        ix = ppac.index(pf["data"], cfg)
        assert ix["n_channels"] == nch and ix["n_blocks"] == len(blks)
        assert np.array_equal(ix["block_start"], pf["block_start"])
        assert ix["block_a"].tolist() == [x["a"] for x in blks] and ix["block_b"].tolist() == [x["b"] for x in blks]
        assert ix["n_samples"] == int(pf["block_start"][-1]) + blks[-1]["a"] + blks[-1]["b"] - dc.settings(sid)["L"]
        offs = ix["chunk_offset"]
        groups = [(True, 0, len(blks) - 1), (False, len(blks) - 1, len(blks))] if nch == 2 else [(False, 0, len(blks))]
        for joint, lo, hi in groups:                             # no chunk is refused: unpack_blocks raises on one
            g = ppac.unpack_blocks(cfg, pf["data"], offs[lo:hi].reshape(-1), nch, joint)
            for i in range(lo, hi):
                k = i - lo
                got = dict(a=int(g["a"][k]), b=int(g["b"][k]), os=g["overall_scale"][k], ms=g["ms_switch"][k],
                           sf=g["scale_factor"][k], ba=g["bit_alloc"][k], mant=g["mantissa"][k])
                _same_integers(got, blks[i], (sid, nch, pf["huffman"], i, blks[i]["name"]))
                assert g["huff_table"][k].tolist() == list(pf["tables"][i])


# ------------------------------------------------------------------------------------------------ d: the PCM condition
@pytest.mark.parametrize("sid", dc.SETTINGS)
def test_no_oracle_sample_sits_on_a_pcm_code_boundary(sid):
    """The GPU file compares 16-bit codes with oracle.decode.pcm16 of the oracle's plane EXACTLY while the planes agree to
    1e-12 of the peak: sound only if no oracle sample lies that close to where the code changes -- (65535 |x| + 1) / 2 at an
    integer for |x| < 1, and |x| = 1 (the clip).  A condition on the input, met by the input (the seeds)."""
    for part, nch in [(part, nch) for part in dc.parts(sid) for nch in (2, 1)]:
        x = np.abs(dc.planes(sid, nch, part)[:, dc.settings(sid)["L"]:])
        tol = BAR * max(float(x.max()), 1.0)
        inside = x[x < 1.0]
        t = (65535.0 * inside + 1.0) / 2.0
        gap = np.abs(t - np.rint(t))
        print("%s %s %dch: peak %.4g, %d samples inside full scale, nearest code boundary %.3g (needs > %.3g), nearest to the clip %.3g"
              % (sid, part, nch, x.max(), inside.size, gap.min(), 65535.0 * tol, np.abs(x - 1.0).min()))
        assert gap.min() > 65535.0 * tol, (sid, part, nch)
        assert np.abs(x - 1.0).min() >= tol, (sid, part, nch)


# ------------------------------------------------------------------------------------------------ e: mutants
def restate_stream(sf, ba, mant, n_scale_bits, sfb, mutation=None):
    """oracle.decode._dequantise_lines / vDequantize (quantize.py:325-357, 90-111), all bands at once"""
    true_cap = (1 << n_scale_bits) - 1
    cap = 15 if mutation == "cap_always_15" else true_cap
    band_of = np.repeat(np.arange(sfb.nBands), sfb.nLines)
    bits = np.asarray(ba, dtype=np.int64)[band_of]
    scale = np.asarray(sf, dtype=np.int64)[band_of]
    m = np.asarray(mant, dtype=np.int64)[:band_of.size]
    on = bits > 0
    safe = np.maximum(bits, 1)
    sign_bit = 1 << (safe - 1)
    if mutation == "sign_threshold_one_bit_off":
        sign_bit = np.maximum(sign_bit >> 1, 1)
    neg = m >= sign_bit
    mag = np.where(neg, m - sign_bit, m)
    n_bits = cap + safe
    shift = cap - scale
    code = (mag << np.maximum(shift, 0)).astype(np.float64)
    half = np.where(shift > 0, 2.0 ** (shift - 1.0), 0.0)
    if mutation == "half_step_at_cap":
        half = np.where(shift == 0, 0.5, half)
    code = code + np.where((mag > 0) | (mutation == "half_step_on_zero_codes"), half, 0.0)
    x = (np.where(neg, -1.0, 1.0) * code) * 2.0 / (2.0 ** n_bits - 1.0)
    return np.where(on, x, 0.0)


def restate_block(p, n_scale_bits, sfb, joint, mutation=None, mid=False):
    """the decoded lines of a parsed block, [nCh][N/2] (mid: [1][N/2]): vDequantize, the overall-scale division
    (codecThem.py:47-51, 92-109), ReconstructLR (ms_stereo.py:33-49) / tests/mix_restatement.py's mid"""
    deq = lambda c: restate_stream(p["sf"][c], p["ba"][c], p["mant"][c], n_scale_bits, sfb, mutation)
    if not joint:
        x = [deq(c) / (1. * (1 << int(p["os"][c]))) for c in range(len(p["ba"]))]
        return [0.5 * (x[0] + x[1])] if mid and len(x) == 2 else x
    band_of = np.repeat(np.arange(sfb.nBands), sfb.nLines)
    lvl = [1. * (1 << int(s)) for s in p["os"]]
    ms = (np.asarray(p["ms"])[:sfb.nBands] == 1)
    if mutation == "switch_ignored_where_a_stream_has_no_bits":
        ms = ms & (np.asarray(p["ba"][0])[:sfb.nBands] > 0) & (np.asarray(p["ba"][1])[:sfb.nBands] > 0)
    ms = ms[band_of]
    m_lvl, s_lvl = lvl[2], lvl[3]
    if mutation == "ms_scales_exchanged":
        m_lvl, s_lvl = s_lvl, m_lvl
    if mutation == "lr_scales_in_ms_bands":
        m_lvl, s_lvl = lvl[0], lvl[1]
    l1 = deq(0) / np.where(ms, m_lvl, lvl[0])
    l2 = deq(1) / np.where(ms, s_lvl, lvl[1])
    if mid:
        return [np.where(ms, l1, (1.0 if mutation == "mid_without_the_half" else 0.5) * (l1 + l2))]
    side = -l2 if mutation == "side_sign_flipped" else l2
    return [np.where(ms, l1 + side, l1), np.where(ms, l1 - side, l2)]


def _synth(lines, a, b, D):
    return RR.synthesise(np.array(lines[:(a + b) // (2 * D)]), a, b, D)


def reduced_lines(lines, a, b, D, mutation=None):
    """the N / (2 D) lines a reduced block synthesises from; the slip: the line past the cut is read too and lands on the last"""
    h = (a + b) // (2 * D)
    x = np.array(lines[:h])
    if mutation == "reduced_reads_one_line_more":
        x[h - 1] += lines[h]
    return x


def parse_any(buf, n_short, blksw):
    """any `.pac` byte string through the oracle's reader -> (cp, [(parsed block, bands, joint)])"""
    cp, off = odec.read_header(buf, n_short, blksw)
    chunks = odec.split_chunks(buf, off)
    nch, out = cp.nChannels, []
    n = len(chunks) // nch
    for i in range(n):
        joint = nch == 2 and i < n - 1
        if joint:
            q = odec.parse_joint_block(chunks[2 * i], chunks[2 * i + 1], cp)
            p = dict(os=q["overallScale"], ms=q["ms_switch"], sf=q["scaleFactor"], ba=q["bitAlloc"], mant=q["mantissa"],
                     table=q["huffTable"])
        else:
            qs = [odec.parse_block(chunks[nch * i + c], cp) for c in range(nch)]
            p = dict(os=[q["overallScale"] for q in qs], ms=None, sf=[q["scaleFactor"] for q in qs], ba=[q["bitAlloc"] for q in qs],
                     mant=[q["mantissa"] for q in qs], table=[q["huffTable"] for q in qs])
        p.update(a=int(cp.a), b=int(cp.b))
        out.append((p, cp.sfBands, joint))
    return cp, out


_PARSED = {}


def _parse_once(key, buf, n_short, blksw):
    if key not in _PARSED:
        _PARSED[key] = parse_any(buf, n_short, blksw)
    return _PARSED[key]


def prepare(cp, parsed):
    """per file, once: every block's lines and mid lines, and the peak of the restated plane at D = 1, 2 and 4"""
    nch = cp.nChannels
    blocks, start = [], 0
    total = sum(p["a"] for p, _, _ in parsed) + parsed[-1][0]["b"]
    ref = {D: np.zeros((nch, total // D)) for D in (1, 2, 4)}
    for p, sfb, joint in parsed:
        good = restate_block(p, cp.nScaleBits, sfb, joint)
        mid = restate_block(p, cp.nScaleBits, sfb, joint, mid=True)[0] if nch == 2 else None
        for D in ref:
            if p["a"] % D == 0 and p["b"] % D == 0 and (p["a"] + p["b"]) % (2 * D) == 0:
                for c in range(nch):
                    ref[D][c, start // D:(start + p["a"] + p["b"]) // D] += _synth(good[c], p["a"], p["b"], D)
        blocks.append((p, sfb, joint, start, good, mid))
        start += p["a"]
    return dict(nch=nch, n_scale_bits=cp.nScaleBits, total=total, blocks=blocks, peak={D: float(np.abs(ref[D]).max()) for D in ref})


def distance(prep, mutation, path):
    """max |mutant's plane - restatement's plane| over the file, as a multiple of BAR x the file's peak, on the path the
    mutation belongs to (lines: the full-rate planes; mid: the one-channel mid, against the stereo peak; reduced: D = 2 and 4).
    The inverse transform being linear, the difference plane is synthesised from the difference of the lines, block by block,
    where they differ at all."""
    nch = prep["nch"]
    if path == "mid" and nch != 2:
        return 0.0
    worst = 0.0
    for D in ((2, 4) if path == "reduced" else (1,)):
        diff = np.zeros((1 if path == "mid" else nch, prep["total"] // D))
        for p, sfb, joint, start, good, mid in prep["blocks"]:
            a, b = p["a"], p["b"]
            if path == "reduced":
                delta = [reduced_lines(g, a, b, D, mutation) - reduced_lines(g, a, b, D) for g in good]
            else:
                bad = restate_block(p, prep["n_scale_bits"], sfb, joint, mutation, mid=path == "mid")
                delta = [x - y for x, y in zip(bad, [mid] if path == "mid" else good)]
            for c, d in enumerate(delta):
                if d.any():
                    diff[c, start // D:(start + a + b) // D] += RR.synthesise(d, a, b, D)
        worst = max(worst, float(np.abs(diff).max() / (BAR * prep["peak"][D])))
    return worst


_PREPARED = {}


def _prepared(key, buf, n_short, blksw):
    if key not in _PREPARED:
        _PREPARED[key] = prepare(*_parse_once(key, buf, n_short, blksw))
    return _PREPARED[key]


def _crafted(everything=True):
    """the raw crafted files, prepared; everything False: without the secondary settings' mono and `full` files (for the mutants:
    they repeat what those settings' stereo main file shows)"""
    out = {}
    for sid in dc.SETTINGS:
        f = dc.settings(sid)
        for pf in dc.files(sid):
            if not pf["huffman"] and (everything or sid in dc.FULL_SETS or (pf["n_channels"] == 2 and pf["part"] == "main")):
                out[pf["label"]] = _prepared(pf["label"], pf["data"], f["S"], f["blksw"])
    return out


def test_restatement_is_the_oracle_bit_for_bit():
    for sid in dc.SETTINGS:
        f = dc.settings(sid)
        for pf in dc.files(sid):
            if pf["huffman"]:
                continue
            prep = _prepared(pf["label"], pf["data"], f["S"], f["blksw"])
            _, want = RR.blocks(pf["data"], f["S"], f["blksw"])
            mids = MR.mid_blocks(pf["data"], f["S"], f["blksw"])[1] if pf["n_channels"] == 2 else None
            assert len(want) == len(prep["blocks"])
            for i, ((p, sfb, joint, start, good, mid), w) in enumerate(zip(prep["blocks"], want)):
                for c in range(prep["nch"]):
                    assert np.array_equal(good[c], w["lines"][c][:good[c].size]), (pf["label"], i, c)
                    assert np.array_equal(np.signbit(good[c]), np.signbit(w["lines"][c][:good[c].size])), (pf["label"], i, c)
                if mids is not None:
                    assert np.array_equal(mid, mids[i]["lines"][:mid.size]), (pf["label"], i, "mid")
            x = dc.planes(sid, pf["n_channels"], pf["part"])
            assert prep["peak"][1] == np.abs(x).max()                      # ... and so is its plane


def test_mutants_are_exposed():
    """Every slip must move a crafted file's plane by more than the bar of its path (a multiple > 1 below).  The table also
    records whether encoder-made kit files see it (the default five-hop stereo file of the store tests and the kit's Huffman
    files at B, E and F): a "no" there is what the crafted files add, a "yes" says the slip is loud enough for any file."""
    crafted = _crafted(everything=False)
    kit = {"default/2ch": _prepared(("kit", "default"), MR.files("default")["files"][0], 128, (1, 1))}
    for sid, nch in (("B", 2), ("E", 2), ("F", 2), ("F", 1)):
        kit["%s/%dch" % (sid, nch)] = _prepared(("kit", sid, nch), SK.oracle_file(sid, nch, True)["data"], SK.lengths(sid)[1], SK.blksw(sid))
    rows = []
    for mutation, path in MUTATIONS.items():
        rows.append((mutation, path, {k: distance(v, mutation, path) for k, v in crafted.items()},
                     {k: distance(v, mutation, path) for k, v in kit.items()}))
    print("\n| mutant | path | crafted files that expose it (largest multiple of the bar) | exposed by encoder-made files |")
    print("|---|---|---|---|")
    for mutation, path, c, k in rows:
        hit, kit_hit = [n for n, v in c.items() if v > 1.0], [n for n, v in k.items() if v > 1.0]
        print("| %s | %s | %d of %d (%.3g at %s) | %s |" % (mutation, path, len(hit), len(c), max(c.values()), max(c, key=c.get),
              ("yes: %d of %d (%.3g)" % (len(kit_hit), len(k), max(k.values()))) if kit_hit else "no"))
    for mutation, path, c, k in rows:
        assert max(c.values()) > 1.0, "no crafted file exposes %s: a family is missing" % mutation
    # a slip that only shows at a cap below 15 shows at the settings that have one, and nowhere at the default setting
    cap15 = dict((m, c) for m, _, c, _ in rows)["cap_always_15"]
    assert max(v for k, v in cap15.items() if k.startswith("default/")) == 0.0
    assert max(v for k, v in cap15.items() if k.startswith("E/")) > 1.0 and max(v for k, v in cap15.items() if k.startswith("F/")) > 1.0
