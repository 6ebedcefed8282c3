"""
The noise-to-mask ratio of mrc_pac_nmr restated in NumPy from the oracle (no tests of its own).

A file's blocks are read as oracle.decode.decode_pac reads them (a stereo file of more than one block: joint blocks, then
Close()'s two non-joint chunks).  Block i of shape (a_i, b_i) covers [p_i, p_i + a_i + b_i) of the channel's padded
source -- n_mdct_lines zeros, the WAV's samples mapped as pcmfile.py:91-100, zeros -- with p_i = a_0 + ... + a_{i-1}.
Per (block, channel) entry and band j:
    noise_j = sum 4 (X - X^)^2      X: windowed MDCT lines of the source block, X^: decoded lines before the IMDCT
    mask_j  = sum 10^((T - 96)/10)  T: masked threshold of the source block (psychoac.py:134-173), dB SPL
    r_j = noise_j / mask_j (0 where mask_j is +inf)
and per file nmr_max_db = 10 log10 max r_j, nmr_total_db = 10 log10(sum_e b_e mean_j r_j / sum_e b_e), disturbed_blocks
(blocks with some channel's r_j > 1) and n_blocks; -inf, -inf, 0, 0 without blocks.
"""
import math
import types

import numpy as np

from oracle import decode as odec, fast


def pcm_to_float(codes):
    """pcmfile.py:91-100: int16 code c -> sign(c) 2|c| / 65535, -32768 -> 0.0"""
    c = np.asarray(codes, dtype=np.float64)
    mag = np.abs(c)
    return np.where(mag >= 32768, 0.0, np.sign(c) * 2.0 * mag / 65535)


def band_sums(X, Xhat, T, n_lines):
    """noise_j, mask_j, r_j of one entry; n_lines: the lines per band."""
    edges = np.concatenate([[0], np.cumsum(n_lines)]).astype(int)
    d = np.asarray(X, np.float64) - np.asarray(Xhat, np.float64)
    noise_line = 4.0 * d * d
    with np.errstate(over="ignore"):
        mask_line = 10.0 ** ((np.asarray(T, np.float64) - 96.0) / 10.0)
    noise = np.array([noise_line[edges[j]:edges[j + 1]].sum() for j in range(len(n_lines))])
    mask = np.array([mask_line[edges[j]:edges[j + 1]].sum() for j in range(len(n_lines))])
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(np.isinf(mask), 0.0, noise / mask)
    return noise, mask, r


def source_analysis(seg, a, b, sample_rate):
    """X (windowed MDCT lines) and T (masked threshold, dB SPL) of one source block of a + b samples (float)."""
    seg = np.asarray(seg, np.float64)[None]
    with np.errstate(over="ignore"):                  # the quiet threshold of the top lines is +inf from ~80 kHz on
        return fast.mdct_batch(seg, a, b)[0], fast.masked_threshold_batch(seg, (a + b) // 2, sample_rate)[0]


def decoded_lines(p, cp, joint):
    """The decoded lines of a parsed block (oracle.decode.parse_block / parse_joint_block dicts, or a list of
    parse_block dicts for non-joint channels) before the IMDCT: [channel][halfN]."""
    if joint:
        lvl = [1. * (1 << int(s)) for s in p["overallScale"]]
        l1 = odec._dequantise_lines(p["scaleFactor"][0], p["bitAlloc"][0], p["mantissa"][0], cp)
        l2 = odec._dequantise_lines(p["scaleFactor"][1], p["bitAlloc"][1], p["mantissa"][1], cp)
        for j in range(cp.sfBands.nBands):
            lo, hi = cp.sfBands.lowerLine[j], cp.sfBands.upperLine[j] + 1
            ms = p["ms_switch"][j] == 1
            if p["bitAlloc"][0][j]:
                l1[lo:hi] /= lvl[2] if ms else lvl[0]
            if p["bitAlloc"][1][j]:
                l2[lo:hi] /= lvl[3] if ms else lvl[1]
        return list(odec.ReconstructLR(l1, l2, cp.sfBands, p["ms_switch"]))
    out = []
    for q in p:
        line = odec._dequantise_lines(q["scaleFactor"], q["bitAlloc"], q["mantissa"], cp)
        out.append(line / (1. * (1 << int(q["overallScale"]))))
    return out


def entry_from_parsed(seg, cp, Xhat, sample_rate):
    """The core on parsed arrays: one entry (source block seg of cp.a + cp.b samples, decoded lines Xhat) ->
    dict(noise, mask, r, peak = max |X|)."""
    X, T = source_analysis(seg, cp.a, cp.b, sample_rate)
    noise, mask, r = band_sums(X, Xhat, T, np.asarray(cp.sfBands.nLines))
    return dict(noise=noise, mask=mask, r=r, peak=float(np.abs(X).max()), X=X, n_lines=np.asarray(cp.sfBands.nLines))


def parse_file(buf, n_short=128, blksw_bits=(1, 1)):
    """-> (cp, nCh, [(a, b, joint, parsed block)]); n_short, blksw_bits: as oracle.decode.read_header"""
    cp, off = odec.read_header(buf, n_short, blksw_bits)
    chunks = odec.split_chunks(buf, off)
    nCh = cp.nChannels
    nBlocks = len(chunks) // nCh
    blocks = []
    for blk in range(nBlocks):
        joint = nCh == 2 and blk < nBlocks - 1
        if joint:
            p = odec.parse_joint_block(chunks[2 * blk], chunks[2 * blk + 1], cp)
        else:
            p = [odec.parse_block(chunks[nCh * blk + ch], cp) for ch in range(nCh)]
        blocks.append((cp.a, cp.b, joint, p, types.SimpleNamespace(a=cp.a, b=cp.b, sfBands=cp.sfBands,
                                                                    nScaleBits=cp.nScaleBits)))
    return cp, nCh, blocks


def restate(buf, pcm, n_short=128, blksw_bits=(1, 1)):
    """One file against its source (int16 [nCh][n], no prior hop) -> dict(entries=[...], shape [E, 2], summaries).
    n_short, blksw_bits: as oracle.decode.read_header."""
    cp, nCh, blocks = parse_file(buf, n_short, blksw_bits)
    L = cp.nMDCTLines
    rate = cp.sampleRate
    pcm = np.atleast_2d(pcm)
    extent = sum(a for (a, _, _, _, _) in blocks) + 2 * L + 2048
    padded = np.zeros((nCh, L + pcm.shape[1] + extent))
    padded[:, L:L + pcm.shape[1]] = pcm_to_float(pcm[:nCh])
    entries, shape = [], []
    start = 0
    for (a, b, joint, p, bcp) in blocks:
        lines = decoded_lines(p, bcp, joint)
        for c in range(nCh):
            e = entry_from_parsed(padded[c, start:start + a + b], bcp, lines[c], rate)
            e["b"] = b
            entries.append(e)
            shape.append((a, b))
        start += a
    return dict(entries=entries, shape=np.array(shape, np.int32).reshape(-1, 2), nch=nCh, **summarise(entries, nCh))


def summarise(entries, nch):
    """entries: dicts with r (per band) and b, ordered by block then channel -> the four per-file numbers."""
    if not entries:
        return dict(nmr_max_db=-math.inf, nmr_total_db=-math.inf, disturbed_blocks=0, n_blocks=0)
    rmax = max(float(np.max(e["r"])) for e in entries)
    num = sum(e["b"] * float(np.mean(e["r"])) for e in entries)
    den = sum(e["b"] for e in entries)
    nblk = len(entries) // nch
    dist = sum(1 for i in range(nblk) if any(np.max(entries[i * nch + c]["r"]) > 1.0 for c in range(nch)))
    db = lambda v: 10.0 * math.log10(v) if v > 0 else -math.inf
    return dict(nmr_max_db=db(rmax), nmr_total_db=db(num / den), disturbed_blocks=dist, n_blocks=nblk)
