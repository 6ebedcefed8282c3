"""
NumPy restatement of the band gains of mrc_pac_store_decode_window_shaped (include/mrc_hip.h), for tests/test_store_shape_cpu.py
and tests/test_gpu_store_shape.py.  A plain module.

The lines are the oracle's: reduced_restatement.blocks (every channel after ReconstructLR) and mix_restatement.mid_blocks (the
mid on the lines).  The band of a line is the stated rule restated here, not the library's answer: with halfN = (a + b) / 2 of
the block's FULL shape, line k lies at f_k = (k + 0.5) * ((sample_rate / halfN) / 2.) and band q holds the lines with
edge[q] <= f_k < edge[q + 1]; a line below edge[0] or at or above the last edge is in no band.  Each line in a band is
multiplied once, in float64, by the band's gain; the others are left as they are.  Then reduced_restatement.synthesise (the
first 1 / D of the lines through the inverse transform and window of the shape (a, b) / D) and the overlap-add of
reduced_restatement.decode, block after block into a zero plane.
"""
import numpy as np

import mix_restatement as MR
import reduced_restatement as RR

NO_BAND = -1


def line_frequencies(sample_rate, a, b):
    half = (a + b) // 2
    return (np.arange(half) + 0.5) * ((float(sample_rate) / half) / 2.)


def line_bands(sample_rate, a, b, edges):
    """-> int64 [(a + b) / 2]: the band of every line of a block of shape (a, b), NO_BAND where it lies in none"""
    f, edges = line_frequencies(sample_rate, a, b), np.asarray(edges, np.float64)
    band = np.full(f.size, NO_BAND, np.int64)
    for q in range(edges.size - 1):
        band[(edges[q] <= f) & (f < edges[q + 1])] = q
    return band


def line_ranges(sample_rate, a, b, edges):
    """-> [bands + 1]: r[q] = the number of lines with f_k < edge[q], so that band q is lines [r[q], r[q + 1])"""
    f = line_frequencies(sample_rate, a, b)
    return np.array([int(np.count_nonzero(f < e)) for e in np.asarray(edges, np.float64)], np.int64)


def shape_lines(lines, sample_rate, a, b, edges, gains):
    """one channel's lines of a block of shape (a, b) with the row of gains applied: one float64 product per line in a band"""
    band = line_bands(sample_rate, a, b, edges)
    inside = band != NO_BAND
    out = np.array(lines, np.float64, copy=True)
    out[inside] = np.asarray(gains, np.float64)[band[inside]] * out[inside]
    return out


def blocks(buf, n_short, blksw_bits, mid=False):
    """the file's blocks with their lines per plane: reduced_restatement.blocks (a plane per channel), or for mid
    mix_restatement.mid_blocks of a stereo file (one plane) -> (planes, [dict(start, a, b, lines [planes][(a + b) / 2], ..)])"""
    if mid:
        _, blks = MR.mid_blocks(buf, n_short, blksw_bits)
        return 1, [dict(k, lines=[k["lines"]]) for k in blks]
    cp, blks = RR.blocks(buf, n_short, blksw_bits)
    return cp.nChannels, blks


def synthesise(planes, blks, D, sample_rate, edges, gains):
    """the blocks of `blocks` with the row `gains` on the bands `edges`, synthesised at 1 / D of the rate and overlap-added as
    reduced_restatement.decode does it -> float64 [planes][samples / D], the MDCT's delay kept as there"""
    total = blks[-1]["start"] + blks[-1]["a"] + blks[-1]["b"]
    plane = np.zeros((planes, total // D))
    for k in blks:
        at, n = k["start"] // D, (k["a"] + k["b"]) // D
        for ch in range(planes):
            plane[ch, at:at + n] += RR.synthesise(shape_lines(k["lines"][ch], sample_rate, k["a"], k["b"], edges, gains), k["a"], k["b"], D)
    return plane


def decode(buf, n_short, blksw_bits, D, sample_rate, edges, gains, mid=False):
    """reduced_restatement.decode (mid: mix_restatement.mid_decode of a stereo file) with the row `gains` on the bands `edges`:
    float64 [nCh][samples / D] (mid: [1][samples / D])"""
    planes, blks = blocks(buf, n_short, blksw_bits, mid)
    return synthesise(planes, blks, D, sample_rate, edges, gains)


# ------------------------------------------------------------------ how exact the restatement itself is
# oracle.decode.IMDCT is the reference's own expression (mdct.py:98-122): exp(1j 2 pi n0 k / N) with k up to N, a phase of up
# to 2 pi n0 ~ 2400 radians that is rounded before it is reduced -- about 1e-13 of the amplitude INSIDE the transform.  For
# a file whose kept samples peak far below that amplitude (a lone block's second half, where its aliasing mostly cancels) this
# can exceed 1e-12 of the file's peak: the restatement then is no reference at that bar.  The same block evaluated exactly --
# the definition x[n] = 2 sum_k X[k] cos(2 pi / N (n + n0)(k + 1 / 2)), the phase reduced in integers, in long double -- says
# how far the restatement lies from what it restates, without any code under test.
_PI = np.longdouble("3.14159265358979323846264338327950288")
_COS = {}


def _cos_matrix(a, b):
    if (a, b) not in _COS:
        if len(_COS) >= 4:
            _COS.clear()
        N = a + b
        n, k = np.arange(N, dtype=np.int64)[:, None], np.arange(N // 2, dtype=np.int64)[None, :]
        m = ((2 * n + b + 1) * (2 * k + 1)) % (4 * N)            # the phase is m pi / (2 N), m exact
        _COS[(a, b)] = np.cos(m.astype(np.longdouble) * (_PI / (2 * N)))
    return _COS[(a, b)]


def synthesise_exact(planes, blks, D, sample_rate, edges, gains):
    """`synthesise` with every block's inverse transform evaluated from its definition in long double (the lines, the band
    rule, the one float64 product per line, the window's float64 values and the overlap-add are the same) -> long double
    [planes][samples / D]"""
    total = blks[-1]["start"] + blks[-1]["a"] + blks[-1]["b"]
    plane = np.zeros((planes, total // D), np.longdouble)
    for k in blks:
        ar, br = k["a"] // D, k["b"] // D
        at, n = k["start"] // D, ar + br
        win = RR.TransitionWindow(np.ones(n), ar, br).astype(np.longdouble)
        for ch in range(planes):
            lines = shape_lines(k["lines"][ch], sample_rate, k["a"], k["b"], edges, gains)[:n // 2]
            plane[ch, at:at + n] += 2 * (_cos_matrix(ar, br) @ lines.astype(np.longdouble)) * win
    return plane
