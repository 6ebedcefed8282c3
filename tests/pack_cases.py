"""
Crafted codes for the `.pac` file layer (the Huffman pricers, the bit writer, the position scan, the chunk parser): what an
encoder seldom produces -- values at and beyond the table edge, every table's escape value, values missing inside a table's
range, 16-bit codes under a forced table, chunks whose tables TIE in price, chunks of every bit length modulo 32.  Pure NumPy
and the oracle; seeded; every product is computed once per configuration and shared (callers must not write into what they
get).

A configuration is (sample rate, n_scale_bits, n_mant_size_bits, a, b, mode); mode is "mono" (one channel, WriteDataBlock),
"split" (two channels, WriteDataBlock: a stereo file's flush block) or "joint" (JointWriteDataBlock).  A chunk is one channel
of one block: the integers bit_alloc [nBands], a DENSE mantissa [N/2] that is zero where the band has no bits, scale_factor
[nBands], and optionally a table id it is forced onto.  A block is one chunk (mono) or two chunks of DIFFERENT families with
the block's overall scales and M/S switch bits.  Every chunk occurs once as channel 0 and, with two channels, once as
channel 1.

No chunk uses a 1-bit allocation: the format stores `ba - 1` (pacfileThem.py:730), a 1 and a 0 are the same header field, so
no reader can tell them apart and a chunk with a 1-bit band cannot round-trip.  (The allocator never grants a single bit
either: bitalloc.py:141-150.)

Every EXPECTED value -- table id, bits_saved, bytes, offsets -- comes from oracle.codec.calculateHuffmanGain and
oracle.pacfile.pack_block / pack_joint_block alone; a forced table's codes from the recoding rule of codecThem.py:194-200 as
tests/test_pack.py spells it out.  The package under test appears only where tests/unpack_corpus._random_blocks draws the
INPUTS of the `mix` family.
"""
import numpy as np

from oracle import codec as ocodec, fast, pacfile as opac
from oracle.huffman_tables import RAW_TABLE_ID, TABLES, TABLE_ORDER

SHAPES = [(1024, 1024), (128, 128), (1024, 128), (128, 1024)]
MODES = ("mono", "split", "joint")
CONFIGS = ([(48000, 4, 4, a, b, mode) for (a, b) in SHAPES for mode in MODES] +
           [(192000, 4, 4, 128, 128, "mono"), (192000, 4, 4, 128, 128, "joint")] +        # bands 0 and 2 hold no lines
           [(44100, 3, 5, 1024, 1024, "joint"), (44100, 3, 5, 1024, 128, "joint")])      # the training script's parameters
TIES = {"tie_raw": None, "tie_01": (0, 1), "tie_12": (1, 2), "tie_23": (2, 3), "tie_023": (0, 2, 3), "tie_all": (0, 1, 2, 3)}
FAMILIES = ("zero", "full16", "escape_value", "lut_edge", "table_holes") + tuple(TIES) + ("single_line", "comb", "phases", "mix")
VARIANTS = ("priced", "raw", "forced")
LONG_BATCH = {"mono": 2051, "joint": 1537}                   # blocks; joint: 3074 chunks = 3 scan tiles + 2 chunks
_CACHE = {}


def config_id(cfg):
    return "%d-s%dm%d-%dx%d-%s" % cfg


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def params(cfg):
    """a fresh oracle CodingParams of the configuration"""
    rate, n_scale, n_mant, a, b, mode = cfg
    cp = ocodec.default_params(sampleRate=rate, nChannels=1 if mode == "mono" else 2)
    cp.nScaleBits, cp.nMantSizeBits = n_scale, n_mant
    cp.a, cp.b = a, b
    cp.sfBands = ocodec.bands_for_block(a, b, cp.nMDCTLines, rate)
    return cp


def layout(cfg):
    def make():
        rate, n_scale, n_mant, a, b, mode = cfg
        cp = params(cfg)
        n_lines = np.asarray(cp.sfBands.nLines, dtype=np.int64)
        nb, half = int(cp.sfBands.nBands), (a + b) // 2
        assert int(n_lines.sum()) == half
        first = 4 + cp.blkswBitA + cp.blkswBitB
        if mode == "joint":
            head = (first + 4 * n_scale + nb, first)         # pacfileThem.py:826-833: scales and switch bits in channel 0 only
        else:
            head = (first + n_scale,) * 2                    # pacfileThem.py:655
        return dict(nb=nb, half=half, n_lines=n_lines, lower=np.concatenate([[0], np.cumsum(n_lines)[:-1]]),
                    band_of=np.repeat(np.arange(nb), n_lines), nch=1 if mode == "mono" else 2, joint=mode == "joint",
                    max_bits=min(16, 1 << n_mant), hb=n_scale + n_mant, head=head, sf_max=(1 << n_scale) - 1,
                    full=np.nonzero(n_lines > 0)[0], has_empty=bool((n_lines == 0).any()))
    return _cached(("layout",) + tuple(cfg), make)


# ------------------------------------------------------------------------------------------------ the oracle's price list
def line_costs(v, ba):
    """codecThem.py:161-173 for one line: what each table charges for value v in a band of ba bits"""
    out = []
    for name in TABLE_ORDER:
        table, esc = TABLES[name]
        out.append(table[v][1] if v in table else ba + table[esc][1])
    return out


def find_tie(winners, max_bits=16):
    """A deterministic search over the oracle's tables, ba ascending, then v1 <= v2 ascending, for (ba, v1, v2) at which the
    tables `winners` and no others share the lowest price of the pair of lines (v1, v2), below the raw 2 ba bits; winners None:
    the lowest price EQUALS the raw size (raw wins the tie).  -> the first match, the first with two different values, the
    first such at 6 bits or wider (where values up to 63 fit) and the first with one value twice, without repeats.  Half the lines of a tying chunk hold v1, half v2."""
    def make():
        found = []
        for ba in range(2, min(max_bits, 7) + 1):
            top = min(1 << ba, 66)
            for v1 in range(top):
                for v2 in range(v1, top):
                    c = [x + y for x, y in zip(line_costs(v1, ba), line_costs(v2, ba))]
                    low = min(c)
                    if winners is None:
                        if low == 2 * ba:
                            found.append((ba, v1, v2))
                    elif low < 2 * ba and tuple(t for t in range(4) if c[t] == low) == tuple(winners):
                        found.append((ba, v1, v2))
        if not found:
            raise AssertionError("no tie of tables %r in the oracle's tables" % (winners,))
        pairs = [f for f in found if f[1] != f[2]]
        out = []
        for f in found[:1] + pairs[:1] + [p for p in pairs if p[0] >= 6][:1] + [f for f in found if f[1] == f[2]][:1]:
            if f not in out:
                out.append(f)
        return out
    return _cached(("tie", winners, max_bits), make)


def holes(t, below=25):
    """values inside table t's range that have no code"""
    table, _ = TABLES[TABLE_ORDER[t]]
    return [v for v in range(min(max(table), below)) if v not in table]


# ------------------------------------------------------------------------------------------------ chunks
def _dense(lay, ba, values):
    """bit_alloc [nb] and per-line values -> the dense plane: zero where the band has no bits; every value must fit its band"""
    ba = np.asarray(ba, dtype=np.int64)
    assert not (ba == 1).any() and ba.min() >= 0 and ba.max() <= lay["max_bits"]
    bits = ba[lay["band_of"]]
    m = np.where(bits > 0, np.asarray(values, dtype=np.int64), 0)
    assert (m >= 0).all() and (m < (1 << bits)).all()
    return ba.astype(np.int32), m.astype(np.int32)


def _cycle(lay, pattern, shift=0):
    return np.asarray(pattern)[(np.arange(lay["nb"]) + shift) % len(pattern)]


def _tie_bands(lay):
    """the first and the last band that hold lines, both sides of a band edge in the middle, and -- so that the two values of
    a pair come equally often -- one more band if the line count is odd"""
    full, n_lines = lay["full"], lay["n_lines"]
    mid = len(full) // 2
    pick = sorted({int(full[0]), int(full[-1]), int(full[mid - 1]), int(full[mid])})
    if sum(n_lines[pick]) % 2:
        odd = [int(b) for b in full if b not in pick and n_lines[b] % 2]
        if not odd:
            raise AssertionError("no band left to make the tying line count even")
        pick.append(odd[0])
    return sorted(pick)


def _phase_chunks(cfg, lay, cp, rng):
    """seeded search: a chunk for every residue modulo 32 of the mantissa bits the writer emits under the priced table (so
    every residue of the chunk's bit count, whatever its header)"""
    cand = lay["full"][:12]
    alphabet = np.array([0, 0, 0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 40])
    got = {}
    for _ in range(6000):
        if len(got) == 32:
            break
        ba = np.zeros(lay["nb"], dtype=np.int64)
        ba[rng.choice(cand, size=int(rng.integers(1, 4)), replace=False)] = rng.integers(2, 9, 3)[0]
        vals = np.minimum(alphabet[rng.integers(0, len(alphabet), lay["half"])], (1 << np.maximum(ba[lay["band_of"]], 1)) - 1)
        ba32, m = _dense(lay, ba, vals)
        t, codes, _ = ocodec.calculateHuffmanGain(fast.compact_mantissa(m, ba32, cp.sfBands), ba32, cp)
        r = int(opac._mantissa_bits(ba32, codes, t, cp.sfBands)) % 32
        if r not in got:
            got[r] = (ba32, m)
    if len(got) != 32:
        raise AssertionError("%s: the search found chunks for %d of 32 bit-count residues" % (config_id(cfg), len(got)))
    return [("phases/mod32_%02d" % r, got[r][0], got[r][1], None) for r in range(32)]


def _chunks(cfg):
    """the named chunks of a configuration: [(name, bit_alloc, mantissa, forced table or None)]"""
    lay, cp = layout(cfg), params(cfg)
    rng = np.random.default_rng([715, cfg[0], cfg[1], cfg[2], cfg[3], cfg[4]])            # (the same chunks in every mode)
    nb, half, top = lay["nb"], lay["half"], lay["max_bits"]
    k = np.arange(half)
    out = []

    def add(name, ba, values, forced=None):
        ba, m = _dense(lay, ba, values)
        out.append((name, ba, m, forced))

    add("zero/all", np.zeros(nb), np.zeros(half))
    # every band at 16 bits (the ones without lines too, as the allocator does): all-ones, sign bit alone, and 1 and 0, which
    # every table codes.  (The largest chunk the format allows is phases/esc22_lead0 below.)
    for forced in (None, 0, 1, 2, 3, RAW_TABLE_ID):
        add("full16/%s" % ("priced" if forced is None else "table%d" % forced), np.full(nb, top),
            np.array([0xFFFF, 0x8000, 0x7FFF, 0x0001, 0])[k % 5] & ((1 << top) - 1), forced)
    # each table's own escape value: priced as its code alone (codecThem.py:169-172), written with the raw bits behind it
    for t, name in enumerate(TABLE_ORDER):
        esc = TABLES[name][1]
        need = esc.bit_length()
        wide = _cycle(lay, [8, need, 2, top, 0], t)
        vals = np.where(wide[lay["band_of"]] >= need, esc, k % 4)
        add("escape_value/%s_wide_priced" % name, wide, vals)
        add("escape_value/%s_wide" % name, wide, vals, t)
        add("escape_value/%s_narrow" % name, np.full(nb, need), np.full(half, esc), t)
    # the edge of the emit table (kPackLutSize 65: 64 is tonal's largest value, 65 the first beyond every table)
    edge_ba = _cycle(lay, [7, 8, top, 12, 0])
    edge = np.stack([np.full(half, 63), np.full(half, 64), np.full(half, 65), np.full(half, 66),
                     (1 << np.maximum(edge_ba[lay["band_of"]], 1)) - 1])[k % 5, k]
    for forced in (None, 0, 1, 2, 3):
        add("lut_edge/%s" % ("priced" if forced is None else "table%d" % forced), edge_ba, edge, forced)
    # ... and the largest coded value where its code length decides the price: zeros and 64s, which only tonal codes
    last = max(v for table, _ in TABLES.values() for v in table)
    add("lut_edge/largest_value_priced", np.full(nb, last.bit_length() + 1), np.where(k % 4 == 0, last, 0))
    union = sorted({v for t in range(4) for v in holes(t)})
    for t, name in enumerate(TABLE_ORDER):
        h = np.asarray(holes(t))
        assert len(h) and h.max() < 32
        add("table_holes/%s" % name, _cycle(lay, [5, 6, 0, top], t), h[k % len(h)], t)
    add("table_holes/union_priced", np.full(nb, 5), np.asarray(union)[k % len(union)])
    # ties: the two values alternate over all lines of the bands with bits, among them line 0, line N/2 - 1 and both sides of a band edge
    bands = _tie_bands(lay)
    for fam, winners in TIES.items():
        for j, (ba, v1, v2) in enumerate(find_tie(winners, top)):
            alloc = np.zeros(nb, dtype=np.int64)
            alloc[bands] = ba
            on = np.nonzero(alloc[lay["band_of"]] > 0)[0]
            vals = np.zeros(half, dtype=np.int64)
            vals[on] = np.where(np.arange(len(on)) % 2 == 0, v1, v2)
            add("%s/ba%d_%d_%d" % (fam, ba, v1, v2), alloc, vals)
    full, n_lines = lay["full"], lay["n_lines"]
    narrow = int(full[np.argmin(n_lines[full])])
    for which, band in (("first", int(full[0])), ("last", int(full[-1])), ("narrowest", narrow)):
        for at, line in (("lo", lay["lower"][band]), ("hi", lay["lower"][band] + n_lines[band] - 1)):
            alloc = np.zeros(nb, dtype=np.int64)
            alloc[band] = 5
            vals = np.zeros(half, dtype=np.int64)
            vals[line] = 17
            add("single_line/%s_%s" % (which, at), alloc, vals, {"lo": None, "hi": len(out) % 4}[at])
    noise = rng.integers(0, 1 << 16, half)
    for name, pattern, forced in (("16_0", [top, 0], None), ("0_16", [0, top], 3), ("2_0", [2, 0], None), ("0_2", [0, 2], 1),
                                  ("0_0_16", [0, 0, top], None), ("0_0_0_2", [0, 0, 0, 2], 0)):
        alloc = _cycle(lay, pattern)
        add("comb/" + name, alloc, noise & ((1 << alloc[lay["band_of"]]) - 1), forced)
    for name, ba, m, forced in _phase_chunks(cfg, lay, cp, rng):
        out.append((name, ba, m, forced))
    # percussive's 6-bit escape code and 16 raw bits on every line, the largest chunk the format allows: 22-bit codes at every
    # bit phase -- after no / one 1-bit code they start at the even / the odd positions
    for lead in (0, 1):
        vals = np.where(k < lead, 0, 0xFFFF - k) & ((1 << top) - 1)
        add("phases/esc22_lead%d" % lead, np.full(nb, top), vals, 0)
    # the longest codes of the tables (9 bits: percussive's 13 and 14) on every line: they start at every bit phase, so a
    # parser's 9-bit look-ahead meets every fill level of its window
    longest = max(n for table, _ in TABLES.values() for (_, n) in table.values())
    nine = [(t, v) for t, name in enumerate(TABLE_ORDER) for v, (_, n) in sorted(TABLES[name][0].items()) if n == longest]
    t9 = nine[0][0]
    v9 = np.asarray([v for (t, v) in nine if t == t9])
    add("phases/longest_code", np.full(nb, max(int(v9.max()).bit_length(), 2)), v9[k % len(v9)], t9)
    out += _mix_chunks(cfg, lay, rng)
    names = [c[0] for c in out]
    assert len(set(names)) == len(names) and {n.split("/")[0] for n in names} == set(FAMILIES)
    return out


def _mix_chunks(cfg, lay, rng):
    import unpack_corpus as UC
    from mrcaudiocodec_amd import pacfile as ppac
    mcfg = ppac.make_config(sample_rate=cfg[0], n_scale_bits=cfg[1], n_mant_size_bits=cfg[2])
    assert list(ppac.band_table(mcfg, cfg[3], cfg[4])) == lay["n_lines"].tolist()
    _, _, _, ba, mant = UC._random_blocks(mcfg, cfg[3], cfg[4], 12, 1, rng)
    out = []
    for i in range(12):
        ba_i, m_i = _dense(lay, ba[i, 0], mant[i, 0])
        out.append(("mix/%02d" % i, ba_i, m_i, [None, None, int(rng.integers(0, 4))][i % 3]))
    return out


# ------------------------------------------------------------------------------------------------ blocks
def cases(cfg):
    """the blocks of a configuration in a seeded random order: dict of overall_scale [n][nch | 4], ms_switch [n][nb] (joint,
    else None), scale_factor / bit_alloc [n][nch][nb], mantissa [n][nch][N/2] int32, forced [n][nch] (-1: none), names
    [n][nch], family [n][nch]"""
    def make():
        lay = layout(cfg)
        chunks = _chunks(cfg)
        nch, nb, n = lay["nch"], lay["nb"], len(chunks)
        rng = np.random.default_rng([716] + [int(v) for v in cfg[:5]] + [MODES.index(cfg[5])])
        fam = [c[0].split("/")[0] for c in chunks]
        order = sorted(range(n), key=lambda i: (FAMILIES.index(fam[i]), i))
        if nch == 2:                                         # channel 1: the chunk one largest-family's length further on
            step = max(fam.count(f) for f in FAMILIES)
            assert 2 * step <= n
            members = [(order[p], order[(p + step) % n]) for p in range(n)]
            assert all(fam[i] != fam[j] for i, j in members)
        else:
            members = [(i,) for i in order]
        members = [members[i] for i in rng.permutation(n)]
        sf_of = {}
        for i in range(n):                                   # per chunk: all 0, all at their maximum, random
            sf_of[i] = [np.zeros(nb, np.int32), np.full(nb, lay["sf_max"], np.int32),
                        rng.integers(0, lay["sf_max"] + 1, nb).astype(np.int32)][min(i % 4, 2)]
        nsc = 4 if lay["joint"] else nch
        osc = rng.integers(0, lay["sf_max"] + 1, (n, nsc)).astype(np.int32)
        osc[0::5], osc[1::5] = 0, lay["sf_max"]
        sw = None
        if lay["joint"]:
            sw = np.stack([[np.zeros(nb, np.int32), np.ones(nb, np.int32), (np.arange(nb) % 2).astype(np.int32)][i % 3]
                           for i in range(n)])
        pick = lambda f, dt: np.array([[f(chunks[i], i) for i in mem] for mem in members], dtype=dt)
        return dict(overall_scale=osc, ms_switch=sw, scale_factor=pick(lambda c, i: sf_of[i], np.int32),
                    bit_alloc=pick(lambda c, i: c[1], np.int32), mantissa=pick(lambda c, i: c[2], np.int32),
                    forced=pick(lambda c, i: -1 if c[3] is None else c[3], np.int32),
                    names=[[chunks[i][0] for i in mem] for mem in members],
                    family=[[fam[i] for i in mem] for mem in members])
    return _cached(("cases",) + tuple(cfg), make)


def recode(compact, t):
    """codecThem.py:194-200 for a GIVEN table: a value with a code gets it, the escape value and every other value the escape
    code followed by the raw mantissa (as tests/test_pack.py::test_pack_with_given_tables_equals_priced spells it out)"""
    if t == RAW_TABLE_ID:
        return compact
    tab, esc = TABLES[TABLE_ORDER[t]]
    return [tab[int(v)][0] if (int(v) in tab and int(v) != esc) else tab[esc][0] + "/" + str(int(v)) for v in compact]


def _pack(cfg, cp, c, i, tables, codes):
    lay = layout(cfg)
    sf, ba = list(c["scale_factor"][i]), list(c["bit_alloc"][i])
    if lay["joint"]:
        return opac.pack_joint_block(sf, ba, codes, [int(v) for v in c["overall_scale"][i]], list(c["ms_switch"][i]), tables, cp)
    return opac.pack_block(sf, ba, codes, [int(v) for v in c["overall_scale"][i]], tables, cp)


def expected(cfg):
    """The oracle on every block, for the three ways of choosing tables -- "priced" (calculateHuffmanGain), "raw" (id 15
    throughout) and "forced" (the chunk's forced table where it has one, else the priced one): table [n][nch], bits_saved
    [n][nch] (priced), blocks[variant] (list of n byte strings), offsets[variant] [n + 1], image[variant] (uint8), and per
    chunk of the priced / forced variants the bits the writer emits: raw_bits, mant_bits[variant], total_bits[variant] [n][nch]"""
    def make():
        lay, cp, c = layout(cfg), params(cfg), cases(cfg)
        n, nch = len(c["names"]), lay["nch"]
        table = {v: np.full((n, nch), RAW_TABLE_ID, np.int32) for v in VARIANTS}
        saved = np.zeros((n, nch), np.int32)
        raw_bits = np.zeros((n, nch), np.int64)
        mant_bits = {v: np.zeros((n, nch), np.int64) for v in VARIANTS}
        blocks = {v: [] for v in VARIANTS}
        for i in range(n):
            codes = {v: [] for v in VARIANTS}
            for ch in range(nch):
                ba = c["bit_alloc"][i, ch]
                compact = fast.compact_mantissa(c["mantissa"][i, ch], ba, cp.sfBands)
                t, priced_codes, sv = ocodec.calculateHuffmanGain(compact, ba, cp)
                f = int(c["forced"][i, ch])
                table["priced"][i, ch], saved[i, ch] = t, sv
                table["forced"][i, ch] = t if f < 0 else f
                codes["priced"].append(priced_codes)
                codes["raw"].append(compact)
                codes["forced"].append(priced_codes if f < 0 else recode(compact, f))
                raw_bits[i, ch] = opac._mantissa_bits(ba, compact, RAW_TABLE_ID, cp.sfBands)
                for v in VARIANTS:
                    mant_bits[v][i, ch] = opac._mantissa_bits(ba, codes[v][ch], int(table[v][i, ch]), cp.sfBands)
            for v in VARIANTS:
                if v == "forced" and (c["forced"][i] < 0).all():
                    blocks[v].append(blocks["priced"][i])
                    continue
                blocks[v].append(_pack(cfg, cp, c, i, [int(t) for t in table[v][i]], codes[v]))
        head = np.asarray(lay["head"][:nch], dtype=np.int64) + lay["nb"] * lay["hb"]
        total_bits = {v: mant_bits[v] + head[None, :] for v in VARIANTS}
        offsets = {v: np.concatenate([[0], np.cumsum([len(b) for b in blocks[v]])]).astype(np.int64) for v in VARIANTS}
        for v in VARIANTS:                                   # the bit counts above are the oracle's own chunk sizes
            assert np.array_equal(np.diff(offsets[v]), (4 + (total_bits[v] + 7) // 8).sum(axis=1)), (config_id(cfg), v)
        image = {v: np.frombuffer(b"".join(blocks[v]), np.uint8) for v in VARIANTS}
        return dict(table=table, bits_saved=saved, blocks=blocks, offsets=offsets, image=image, raw_bits=raw_bits,
                    mant_bits=mant_bits, total_bits=total_bits)
    return _cached(("expected",) + tuple(cfg), make)


def chunk_offsets(cfg, variant):
    """where every chunk's length field lies in image[variant]: int64 [n * nch], as the parsers take them"""
    lay, e = layout(cfg), expected(cfg)
    per = 4 + (e["total_bits"][variant] + 7) // 8
    start = e["offsets"][variant][:-1, None] + np.concatenate([np.zeros((len(per), 1), np.int64), np.cumsum(per, axis=1)[:, :-1]], axis=1)
    return np.ascontiguousarray(start.reshape(-1), dtype=np.int64)


def table_costs(cfg, i, ch):
    """the oracle's price of block i's channel ch under each table (untruncated where it matters: a price above the raw size
    may stop early, codecThem.py:159) and the raw size"""
    cp, c = params(cfg), cases(cfg)
    ba = c["bit_alloc"][i, ch]
    compact = fast.compact_mantissa(c["mantissa"][i, ch], ba, cp.sfBands)
    raw = int(opac._mantissa_bits(ba, compact, RAW_TABLE_ID, cp.sfBands))
    return [int(ocodec.huffman_cost(compact, ba, cp.sfBands, TABLES[name][0], TABLES[name][1], raw)) for name in TABLE_ORDER], raw


def code_spans(cfg, i, ch, variant):
    """(first bit, length) of every line's code in block i's channel ch, counted from the chunk's first payload bit, from the
    oracle's code strings"""
    lay, cp, c, e = layout(cfg), params(cfg), cases(cfg), expected(cfg)
    ba = c["bit_alloc"][i, ch]
    t = int(e["table"][variant][i, ch])
    codes = recode(fast.compact_mantissa(c["mantissa"][i, ch], ba, cp.sfBands), t)
    esc = None if t == RAW_TABLE_ID else TABLES[TABLE_ORDER[t]][0][TABLES[TABLE_ORDER[t]][1]][0]
    at, j, out = lay["head"][ch], 0, []
    for band in range(lay["nb"]):
        at += lay["hb"]
        if ba[band]:
            for _ in range(int(lay["n_lines"][band])):
                if esc is None:
                    n = int(ba[band])
                else:
                    head = str(codes[j]).split("/")[0]
                    n = len(head) + (int(ba[band]) if head == esc else 0)
                out.append((at, n))
                at += n
                j += 1
    assert at == e["total_bits"][variant][i, ch]
    return out


# ------------------------------------------------------------------------------------------------ the long batches
def long_batch(mode):
    """the (128,128) case list at 48 kHz repeated cyclically over LONG_BATCH[mode] blocks, tables priced: dict of cfg, index
    [N] (into the case list), image (uint8), offsets [N + 1], table / bits_saved [N][nch], chunk_offsets [N * nch]"""
    def make():
        cfg = (48000, 4, 4, 128, 128, mode)
        e = expected(cfg)
        n = len(e["blocks"]["priced"])
        idx = np.arange(LONG_BATCH[mode]) % n
        size = np.diff(e["offsets"]["priced"])[idx]
        offsets = np.concatenate([[0], np.cumsum(size)]).astype(np.int64)
        rel = (chunk_offsets(cfg, "priced").reshape(n, -1) - e["offsets"]["priced"][:-1, None])[idx]
        return dict(cfg=cfg, index=idx, image=np.frombuffer(b"".join(e["blocks"]["priced"][i] for i in idx), np.uint8),
                    offsets=offsets, table=e["table"]["priced"][idx], bits_saved=e["bits_saved"][idx],
                    chunk_offsets=np.ascontiguousarray((rel + offsets[:-1, None]).reshape(-1)))
    return _cached(("long", mode), make)


def first_difference(cfg, variant, got, names=None, offsets=None, want=None):
    """None if the uint8 array `got` is expected(cfg)'s image[variant] (or `want`, with its block offsets and names), else a
    sentence naming the first differing byte and the block (its chunks' names) it lies in"""
    e = expected(cfg)
    want = e["image"][variant] if want is None else want
    offsets = e["offsets"][variant] if offsets is None else offsets
    names = cases(cfg)["names"] if names is None else names
    got = np.asarray(got, dtype=np.uint8).reshape(-1)
    n = min(got.size, want.size)
    diff = np.nonzero(got[:n] != want[:n])[0]
    if not diff.size and got.size == want.size:
        return None
    at = int(diff[0]) if diff.size else n
    blk = min(int(np.searchsorted(offsets, at, side="right")) - 1, len(names) - 1)
    return "%s %s: %d bytes, %d expected; first differing byte %d (block %d %r, byte %d of it): got %s, expected %s" % (
        config_id(cfg), variant, got.size, want.size, at, blk, names[blk], at - int(offsets[blk]),
        got[at] if at < got.size else None, want[at] if at < want.size else None)


def parsed(cfg, variant):
    """what a chunk parser must return for image[variant], in the fixed-stride layout of mrc_unpack_blocks (32 bands, nMDCTLines
    lines): the crafted integers themselves"""
    lay, c, e = layout(cfg), cases(cfg), expected(cfg)
    n, nch, nb, half = len(c["names"]), lay["nch"], lay["nb"], lay["half"]
    pad = lambda x, width: np.concatenate([x, np.zeros(x.shape[:-1] + (width - x.shape[-1],), np.int32)], axis=-1)
    return dict(a=np.full(n, cfg[3], np.int32), b=np.full(n, cfg[4], np.int32), huff_table=e["table"][variant],
                overall_scale=c["overall_scale"], ms_switch=pad(c["ms_switch"], 32) if lay["joint"] else None,
                scale_factor=pad(c["scale_factor"], 32), bit_alloc=pad(c["bit_alloc"], 32), mantissa=pad(c["mantissa"], 1024))


def parsed_difference(cfg, variant, got, want=None, names=None):
    """None if a parser's arrays `got` are parsed(cfg, variant) (or `want`), else a sentence naming the first differing field"""
    want = parsed(cfg, variant) if want is None else want
    names = cases(cfg)["names"] if names is None else names
    for k, v in want.items():
        if v is None:
            continue                              # (ms_switch: left alone for independent channels)
        g = np.asarray(got[k])
        if g.shape != v.shape:
            return "%s %s: %s has shape %r, expected %r" % (config_id(cfg), variant, k, g.shape, v.shape)
        bad = np.argwhere(g != v)
        if len(bad):
            at = tuple(bad[0])
            return "%s %s: %s differs in block %d %r at %s: got %d, expected %d" % (
                config_id(cfg), variant, k, at[0], names[at[0] % len(names)], tuple(int(x) for x in at[1:]), g[at], v[at])
    return None
