"""
The codec settings the file-level tests run at besides the default (tests/test_settings_cpu.py on the CPU,
tests/test_gpu_settings_files.py on the GPU): per setting the Handle arguments, the matching pacfile.make_config and
oracle CodingParams, one short int16 stereo stream (its left channel is the mono stream) with the zero prior hop, block
schedules that pass through every block shape of the setting, and the oracle's files of them with every integer the oracle
wrote.  A plain module; everything oracle-side is computed once per process and handed out read-only.

The signal of a setting is chosen so that its Huffman-coded stereo file holds chunks with a table id in 0..3 AND raw
chunks (tests/test_settings_cpu.py asserts it on the oracle alone).  Where the oracle never picks both at a setting,
HUFFMAN_FORCED names the setting and the Huffman decode is covered there by host-packed chunks with forced tables
(forced_table_cases).  COVERS lists, per setting, which items of the GPU file run at it.
"""
import numpy as np

from oracle import codec as ocodec, decode as odec, pacfile as opac
from oracle.huffman_tables import RAW_TABLE_ID

# id -> (Handle keyword arguments, why the setting is here)
SETTINGS = {
    "B": (dict(n_mdct_lines=512, n_short=256), "generic decode and MDCT sizes; store margins with L != 1024"),
    "C": (dict(n_mdct_lines=256, n_short=128), "25 bands over 256 lines, many one-line bands"),
    "D": (dict(n_mdct_lines=1024, n_short=512), "joint transition block of 1536 coded lines (chained limit 2048)"),
    "E": (dict(n_scale_bits=3, n_mant_size_bits=5, sample_rate=44100, target_bits_per_sample=2.27),
          "the reference's training settings"),
    "F": (dict(n_scale_bits=1, n_mant_size_bits=3), "scale factor -1; maxMantBits 8"),
    "G": (dict(n_scale_bits=2, n_mant_size_bits=8), "widest allocation field"),
    "H": (dict(n_mant_size_bits=1), "maxMantBits 2: K = 1, VBR candidates {0, 2}"),
    "I": (dict(blksw_bits_a=2, blksw_bits_b=2), "two-bit block-switch fields"),
    "J": (dict(blksw_bits_a=0, blksw_bits_b=0), "no block-switch fields: long blocks only"),
    "K": (dict(n_mdct_lines=768, n_short=384), "a block length with a factor 3 (the header reader)"),
}
IDS = sorted(SETTINGS)
_DEFAULTS = dict(sample_rate=48000, n_mdct_lines=1024, n_short=128, n_scale_bits=4, n_mant_size_bits=4,
                 target_bits_per_sample=2.86, blksw_bits_a=1, blksw_bits_b=1)
REFUSED_LENGTHS = [(512, 128), (1024, 256)]       # Handle() refuses them: "block length must factor into 2s and 3s"

# which items of tests/test_gpu_settings_files.py run at a setting (1 stereo, 2 mono, 3 ladder, 4 device packer / parser,
# 5 whole-file decode, 6 store, 7 NMR, 8 VBR and target-NMR, 9 block-switch width 0)
COVERS = {sid: {1, 2, 4, 5, 7} for sid in IDS}
for _s in "BEFH":
    COVERS[_s].add(3)
for _s in "BCDK":
    COVERS[_s].add(6)
for _s in "BCFH":
    COVERS[_s].add(8)
COVERS["J"].add(9)

# per setting: (seed, tone amplitude, noise sigma of the loud half, noise sigma of the quiet half)
_SIGNAL = {sid: (20 + i, 0.25, 0.05, 2e-4) for i, sid in enumerate(IDS)}
_SIGNAL.update(C=(21, 0.9, 0.003, 0.003),     # (the default mix: every chunk raw at C, H and J, every chunk on a table at F)
               F=(24, 0.25, 0.3, 2e-4), H=(26, 0.25, 0.3, 0.0), J=(28, 0.9, 0.05, 2e-4))
# Settings at which the oracle picks no table, or no raw chunk, for any signal tried: none -- with the mixes above every
# setting's Huffman file holds both (asserted in tests/test_settings_cpu.py).  forced_table_cases() still runs at every setting:
# the oracle's choice never covers all four table ids at one setting.
HUFFMAN_FORCED = ()

_CACHE = {}


def handle_kwargs(sid):
    return dict(SETTINGS[sid][0])


def full(sid):
    """every codec argument of the setting, defaults filled in"""
    return dict(_DEFAULTS, **SETTINGS[sid][0])


def config(sid):
    from mrcaudiocodec_amd import pacfile as ppac
    return ppac.make_config(**full(sid))


def lengths(sid):
    f = full(sid)
    return f["n_mdct_lines"], f["n_short"]


def blksw(sid):
    f = full(sid)
    return f["blksw_bits_a"], f["blksw_bits_b"]


def max_mant_bits(sid):
    return min(16, 1 << full(sid)["n_mant_size_bits"])


def coding_params(sid, n_channels, bits_per_sample=None):
    """a fresh oracle CodingParams of the setting (the encoders write into it)"""
    f = full(sid)
    cp = ocodec.default_params(sampleRate=f["sample_rate"], nChannels=n_channels,
                               targetBitsPerSample=f["target_bits_per_sample"] if bits_per_sample is None else bits_per_sample)
    cp.nMDCTLines = cp.nSamplesPerBlock = cp.a = cp.b = f["n_mdct_lines"]
    cp.nSamplesShort = f["n_short"]
    cp.nScaleBits, cp.nMantSizeBits = f["n_scale_bits"], f["n_mant_size_bits"]
    cp.blkswBitA, cp.blkswBitB = f["blksw_bits_a"], f["blksw_bits_b"]
    cp.sfBands = ocodec.bands_for_block(cp.a, cp.b, cp.nMDCTLines, cp.sampleRate)
    cp.bitReservoir = 0
    return cp


def _chain(ab):
    offs = np.concatenate([[0], np.cumsum([a for a, _ in ab])[:-1]])
    return [(int(o), int(a), int(b)) for o, (a, b) in zip(offs, ab)]


def schedule(sid, which=0):
    """[(offset, a, b)]: (L,L), (L,S), (S,S).., (S,L), (L,L) with the (S,S) run a hop long -- which = 1: the switch one
    block earlier and two long blocks at the end (another schedule over the same stream).  Setting J: long blocks only."""
    L, S = lengths(sid)
    if sid == "J":
        return _chain([(L, L)] * (6 if which == 0 else 5))
    run = [(L, S)] + [(S, S)] * (L // S - 1) + [(S, L)]
    return _chain(([(L, L)] * 2 + run + [(L, L)]) if which == 0 else ([(L, L)] + run + [(L, L)] * 2))


def shapes_of(sid):
    L, S = lengths(sid)
    return [(L, L)] if sid == "J" else [(L, L), (L, S), (S, S), (S, L)]


def n_hops(sid):
    return 6 if sid == "J" else 5


def stream(sid):
    """int16 [2][(hops + 1) L], the first hop zero.  A tone common to both channels (M/S bands) over independent noise (L/R
    bands): loud noise in the first half (large codes: raw chunks), next to none in the second (small codes: a table)."""
    key = ("stream", sid)
    if key not in _CACHE:
        L, _ = lengths(sid)
        seed, amp, loud, quiet = _SIGNAL[sid]
        rate = full(sid)["sample_rate"]
        n = n_hops(sid) * L
        rng = np.random.default_rng(seed)
        t = np.arange(n)
        tone = amp * np.sin(2 * np.pi * 1000.0 / rate * t) + 0.3 * amp * np.sin(2 * np.pi * 5200.0 / rate * t)
        sigma = np.where(t < n // 2, loud, quiet)
        x = tone[None] + sigma[None] * rng.standard_normal((2, n))
        pcm = np.zeros((2, n + L), np.int16)
        pcm[:, L:] = np.clip(np.rint(x * 32767.5), -32767, 32767).astype(np.int16)
        pcm.setflags(write=False)
        _CACHE[key] = pcm
    return _CACHE[key]


def mono(sid):
    return stream(sid)[:1]


def to_float(pcm):
    """pcmfile.py:91-100, as the library maps int16 codes"""
    c = np.asarray(pcm, dtype=np.float64)
    mag = np.abs(c)
    return np.where(mag >= 32768, 0.0, np.sign(c) * 2.0 * mag / 65535)


def source(sid, n_channels, shapes=None):
    """what mrc_pac_nmr measures a file against: the stream from the end of the prior hop to the end of its last block"""
    L, _ = lengths(sid)
    o, a, b = (schedule(sid) if shapes is None else shapes)[-1]
    return np.ascontiguousarray(stream(sid)[:n_channels, L:o + a + b])


# ------------------------------------------------------------------ the oracle's files, with the integers behind them
def _expand(compact, ba, sfb, half):
    """the compact mantissa list of the oracle -> the dense plane the library takes"""
    out = np.zeros(half, np.int32)
    i = 0
    for j in range(sfb.nBands):
        n = int(sfb.nLines[j])
        if ba[j]:
            out[int(sfb.lowerLine[j]):int(sfb.lowerLine[j]) + n] = compact[i:i + n]
            i += n
    return out


def oracle_file(sid, n_channels, huffman, which=0, bits_per_sample=None):
    """The oracle's `.pac` file of the setting's stream on schedule `which` -- oracle.pacfile.encode_stereo_stream /
    tests/mono_oracle.encode_mono_stream, spelled out block by block so that the integers are kept -> dict: data (bytes),
    blocks = [dict(a, b, joint, nch, os, ms, sf, ba (lists per coded stream), mant (dense int32 per stream), table,
    chunk (the block's bytes))], Close()'s block last.  Read-only."""
    key = ("file", sid, n_channels, bool(huffman), which, bits_per_sample)
    if key in _CACHE:
        return _CACHE[key]
    cp = coding_params(sid, n_channels, bits_per_sample)
    L = cp.nMDCTLines
    shapes = schedule(sid, which)
    x = to_float(stream(sid)[:n_channels])
    out = [opac.file_header(cp, sum(b for (_, _, b) in shapes))]
    blocks = []

    def independent(segs, a, b):
        cp.a, cp.b = a, b
        cp.sfBands = ocodec.bands_for_block(a, b, L, cp.sampleRate)
        sf, ba, codes, osc, tabs, dense = [], [], [], [], [], []
        for seg in segs:                                       # codec.Encode / EncodeNoHuff, channel after channel
            s, al, m, o = ocodec.EncodeSingleChannel(seg, cp)
            t, c, saved = ocodec.calculateHuffmanGain(m, al, cp) if huffman else (RAW_TABLE_ID, m, 0)
            cp.bitReservoir += saved
            sf.append(np.array(s)); ba.append(np.array(al)); codes.append(c); osc.append(int(o)); tabs.append(int(t))
            dense.append(_expand(m, al, cp.sfBands, (a + b) // 2))
        chunk = opac.pack_block(sf, ba, codes, osc, tabs, cp)
        blocks.append(dict(a=a, b=b, joint=False, nch=len(segs), os=osc, ms=None, sf=sf, ba=ba, mant=dense, table=tabs,
                           chunk=chunk, bands=cp.sfBands))
        out.append(chunk)

    for (off, a, b) in shapes:
        if n_channels == 1:
            independent([x[0, off:off + a + b].copy()], a, b)
            continue
        cp.a, cp.b = a, b
        cp.sfBands = ocodec.bands_for_block(a, b, L, cp.sampleRate)
        sf, ba, m, osc, sw = ocodec.JointEncodeChannels(x[0, off:off + a + b].copy(), x[1, off:off + a + b].copy(), cp)
        codes, tabs = [], []
        for c in range(2):                                     # codec.JointEncode's Huffman stage
            t, cd, saved = ocodec.calculateHuffmanGain(m[c], ba[c], cp) if huffman else (RAW_TABLE_ID, m[c], 0)
            cp.bitReservoir += saved
            codes.append(cd); tabs.append(int(t))
        chunk = opac.pack_joint_block(sf, ba, codes, osc, sw, tabs, cp)
        blocks.append(dict(a=a, b=b, joint=True, nch=2, os=[int(v) for v in osc], ms=np.array(sw), sf=[np.array(v) for v in sf],
                           ba=[np.array(v) for v in ba], mant=[_expand(m[c], ba[c], cp.sfBands, (a + b) // 2) for c in range(2)],
                           table=tabs, chunk=chunk, bands=cp.sfBands))
        out.append(chunk)
    off, a, b = shapes[-1]                                       # Close(): the last hop and L zeros, non-joint
    independent([np.concatenate([x[c, off + a:off + a + b], np.zeros(L)]) for c in range(n_channels)], L, L)
    res = dict(data=b"".join(out), blocks=blocks, shapes=shapes)
    _CACHE[key] = res
    return res


def oracle_decode(sid, data):
    """oracle.decode.decode_pac of a file of the setting -> float64 [nCh][samples] (read-only, cached by content)"""
    key = ("decode", sid, data)
    if key not in _CACHE:
        x = odec.decode_pac(data, lengths(sid)[1], blksw(sid))[1]
        x.setflags(write=False)
        _CACHE[key] = x
    return _CACHE[key]


def block_arrays(blocks):
    """blocks of ONE shape and kind from oracle_file -> the arrays pack_blocks / pack_joint_blocks take:
    (overall_scale [n][4 | nch], ms_switch [n][nb] | None, scale_factor, bit_alloc [n][nch][nb], mantissa [n][nch][half])"""
    osc = np.array([b["os"] for b in blocks], np.int32)
    ms = np.array([b["ms"] for b in blocks], np.int32) if blocks[0]["joint"] else None
    sf = np.array([np.stack(b["sf"]) for b in blocks], np.int32)
    ba = np.array([np.stack(b["ba"]) for b in blocks], np.int32)
    mant = np.array([np.stack(b["mant"]) for b in blocks], np.int32)
    return osc, ms, sf, ba, mant


def forced_table_cases(sid, seed=0):
    """chunk sets of the setting with every Huffman table forced (host packer, pack_blocks(..., huff_table=)), independent
    and joint, every shape: dicts as tests/unpack_corpus.py's cases"""
    from mrcaudiocodec_amd import pacfile as ppac
    import unpack_corpus as UC
    cfg = config(sid)
    rng = np.random.default_rng(1000 + seed + ord(sid))
    out = []
    for (a, b) in shapes_of(sid):
        osc, sw, sf, ba, mant = UC._random_blocks(cfg, a, b, 4, 2, rng)
        head = ppac.header(cfg, 2, 4 * b)
        for t in (0, 1, 2, 3, 15):
            tab = np.full((4, 2), t, np.int32)
            for joint in (False, True):
                if joint:
                    d = ppac.pack_joint_blocks(cfg, a, b, osc, sw, sf, ba, mant, True, huff_table=tab)[0]
                else:
                    d = ppac.pack_blocks(cfg, a, b, osc[:, :2], sf, ba, mant, True, huff_table=tab)[0]
                blob = head + d.tobytes()
                out.append(dict(cfg=cfg, buf=blob, offsets=ppac.scan_chunks(blob, len(head)), nch=2, joint=joint,
                                label="%s_%stable%d_%d_%d" % (sid, "j" if joint else "", t, a, b)))
    return out


def file_cases(sid):
    """the oracle's four files of the setting (stereo / mono, Huffman / raw) as chunk-parser cases"""
    import unpack_corpus as UC
    out = []
    for nch in (2, 1):
        for huff in (True, False):
            out += UC._file_cases(oracle_file(sid, nch, huff)["data"], "%s_%dch_huff%d" % (sid, nch, huff), config(sid))
    return out
