"""
The reduced-rate decode of a `.pac` file, restated in NumPy from the oracle's own functions (oracle.decode.read_header,
split_chunks, parse_block, parse_joint_block, _dequantise_lines, ReconstructLR, IMDCT and oracle.window.TransitionWindow):
what mrc_pac_store_decode_window_reduced is held against.  A plain module.

A block of shape (a, b), N = a + b, decodes at 1 / D of the sample rate as the IMDCT of shape (a / D, b / D) of its first
N / (2 D) lines under the transition window of that shape.  With n0 = (b + 1) / 2 and n0' = (b / D + 1) / 2,
(n + n0) / N = (m + n0') / (N / D) exactly when n = D m + (D - 1) / 2, and the oracle's IMDCT carries no factor that
depends on N: the reduced block is the band-limited full block at those times, unscaled.  Blocks are added into a zero plane
in file order, block i at block_start[i] / D.  At D = 1 this is oracle.decode.decode_pac bit for bit.
"""
import numpy as np

from oracle import decode as odec
from oracle.window import TransitionWindow


def _lines(cp, chunks, blk, joint):
    """the dequantised, rescaled, L/R-reconstructed lines of block blk, one full-length array per channel, and its parse;
    sets cp.a, cp.b, cp.sfBands as the oracle's readers do"""
    nCh = cp.nChannels
    if not joint:
        out, parses = [], []
        for ch in range(nCh):
            p = odec.parse_block(chunks[nCh * blk + ch], cp)
            line = odec._dequantise_lines(p["scaleFactor"], p["bitAlloc"], p["mantissa"], cp)
            line /= 1. * (1 << p["overallScale"])                                   # Decode
            out.append(line)
            parses.append(p)
        return out, parses
    p = odec.parse_joint_block(chunks[2 * blk], chunks[2 * blk + 1], cp)
    lvl = [1. * (1 << int(s)) for s in p["overallScale"]]                           # JointDecode
    l1 = odec._dequantise_lines(p["scaleFactor"][0], p["bitAlloc"][0], p["mantissa"][0], cp)
    l2 = odec._dequantise_lines(p["scaleFactor"][1], p["bitAlloc"][1], p["mantissa"][1], cp)
    for iBand in range(cp.sfBands.nBands):
        lo, hi = cp.sfBands.lowerLine[iBand], cp.sfBands.upperLine[iBand] + 1
        ms = p["ms_switch"][iBand] == 1
        if p["bitAlloc"][0][iBand]:
            l1[lo:hi] /= lvl[2] if ms else lvl[0]
        if p["bitAlloc"][1][iBand]:
            l2[lo:hi] /= lvl[3] if ms else lvl[1]
    return list(odec.ReconstructLR(l1, l2, cp.sfBands, p["ms_switch"])), [p]


def blocks(buf, n_short, blksw_bits):
    """-> (cp, [dict(start, a, b, joint, lines [nCh][(a + b) / 2], ms (the joint block's switches or None))]) in file order"""
    cp, off = odec.read_header(buf, n_short, blksw_bits)
    chunks = odec.split_chunks(buf, off)
    nCh = cp.nChannels
    if len(chunks) % nCh:
        raise ValueError("chunk count is not a multiple of the channel count")
    n, out, start = len(chunks) // nCh, [], 0
    for blk in range(n):
        joint = nCh == 2 and blk < n - 1
        lines, parses = _lines(cp, chunks, blk, joint)
        out.append(dict(start=start, a=int(cp.a), b=int(cp.b), joint=joint, lines=lines,
                        ms=np.array(parses[0]["ms_switch"]) if joint else None))
        start += int(cp.a)
    return cp, out


def synthesise(lines, a, b, D):
    """one channel's block at 1 / D of the rate: the windowed (a + b) / D samples, before overlap-and-add"""
    ar, br = a // D, b // D
    if ar * D != a or br * D != b:
        raise ValueError("block shape (%d,%d) does not divide by %d" % (a, b, D))
    return TransitionWindow(odec.IMDCT(lines[:(ar + br) // 2], ar, br), ar, br)


def decode(buf, n_short, blksw_bits, D):
    """-> float64 [nCh][samples / D], samples = last block's start + a + b: the MDCT's delay (the first n_mdct_lines / D
    samples) kept, as oracle.decode.decode_pac keeps it"""
    cp, blks = blocks(buf, n_short, blksw_bits)
    if not blks:
        return np.zeros((cp.nChannels, cp.nMDCTLines // D))
    total = blks[-1]["start"] + blks[-1]["a"] + blks[-1]["b"]
    plane = np.zeros((cp.nChannels, total // D))
    for k in blks:
        at, n = k["start"] // D, (k["a"] + k["b"]) // D
        for ch in range(cp.nChannels):
            plane[ch, at:at + n] += synthesise(k["lines"][ch], k["a"], k["b"], D)
    return plane
