"""
mrc_band_line_ranges and mrc_pac_store_band_energy_window restated in NumPy, in the library's stated order, on the decoded
lines of tests/reduced_restatement.blocks and tests/mix_restatement.mid_blocks (tests/test_store_bands_cpu.py,
tests/test_gpu_store_bands.py).  A plain module.

    line k of a block of shape (a, b) lies at f_k = (k + 0.5) * ((fs / halfN) / 2.), halfN = (a + b) / 2 (psychoac.py:94);
    line_lo[q] = #{k : f_k < edge[q]} (psychoac.py:99); band q holds lines [line_lo[q], line_lo[q + 1]);
    B[q] = the left fold from +0.0 over k ascending of lines[k] ** 2 (a square rounded once, then added);
    block n's tile, doubled: [2 p + a - 2 L, 2 p + 2 a + b - 2 L); frame j, doubled: [2 (start + j hop), 2 (start + (j + 1) hop));
    out[q][j] = the left fold from +0.0 over the blocks in ascending order with ov2 > 0 of float(ov2) * B_n[q].

Overlaps are Python integers: nothing overflows, whatever the start.
"""
import numpy as np

import mix_restatement as MR
import reduced_restatement as RR

# psychoac.py:82-84 without the last limit, as mrcaudiocodec_amd.store.CRITICAL_BAND_LIMITS_HZ has them
CRITICAL_LIMITS = (100, 200, 300, 400, 510, 630, 770, 920, 1080, 1270, 1480, 1720, 2000, 2320, 2700, 3150, 3700, 4400, 5300, 6400,
                   7700, 9500, 12000, 15500)


def critical_edges(fs):
    return np.array([0.0] + [float(f) for f in CRITICAL_LIMITS if f < fs / 2.0] + [fs / 2.0])


def narrow_edges(fs):
    """40 bands from 50 Hz to 0.4 fs in equal ratios: the lowest are a few Hz wide, narrower than any block's line spacing"""
    return np.geomspace(50.0, 0.4 * fs, 41)


def line_ranges(fs, a, b, edges):
    """-> int32 [len(edges)]: the number of lines of a block of shape (a, b) that lie below each edge"""
    halfN = (a + b) // 2
    f = (np.arange(halfN) + 0.5) * ((float(fs) / halfN) / 2.)
    return np.array([int(np.count_nonzero(f < e)) for e in np.asarray(edges, dtype=np.float64)], dtype=np.int32)


def band_sums(lines, lo):
    """B [len(lo) - 1] of one block's lines: np.add.accumulate is the sequential left fold, and +0.0 + v == v"""
    sq = np.asarray(lines, dtype=np.float64) ** 2
    out = np.zeros(len(lo) - 1)
    for q in range(len(lo) - 1):
        if lo[q + 1] > lo[q]:
            out[q] = np.add.accumulate(sq[lo[q]:lo[q + 1]])[-1]
    return out


def tile2(start, a, b, L):
    """a block's tile in doubled output samples"""
    return 2 * start + a - 2 * L, 2 * start + 2 * a + b - 2 * L


def frames(blocks, B, L, start, n_frames, hop):
    """blocks [(p, a, b)] in file order, B [n_blocks][n_bands] -> (out float64 [n_bands][n_frames], the indices of the blocks
    whose tile overlaps [start, start + n_frames hop): the blocks the call parses)"""
    start, n_frames, hop = int(start), int(n_frames), int(hop)
    B = np.asarray(B, dtype=np.float64).reshape(len(blocks), -1)
    out = np.zeros((B.shape[1], n_frames))
    tiles = [tile2(int(p), int(a), int(b), L) for p, a, b in blocks]
    needed = [n for n, (t0, t1) in enumerate(tiles) if min(t1, 2 * (start + n_frames * hop)) - max(t0, 2 * start) > 0]
    for j in range(n_frames):
        f0, f1 = 2 * (start + j * hop), 2 * (start + (j + 1) * hop)
        acc = np.zeros(B.shape[1])
        for n in needed:
            ov2 = min(tiles[n][1], f1) - max(tiles[n][0], f0)
            if ov2 > 0:
                acc = acc + float(ov2) * B[n]
        out[:, j] = acc
    return out, needed


class FileBands:
    """one file's blocks and decoded lines, per channel and (stereo) of the mid, parsed once; B per (edges, what) on demand"""

    def __init__(self, buf, n_short, blksw_bits, L, fs):
        self.L, self.fs = int(L), fs
        cp, blks = RR.blocks(buf, n_short, blksw_bits)
        self.nch = cp.nChannels
        self.blocks = [(k["start"], k["a"], k["b"]) for k in blks]
        self.lines = {c: [k["lines"][c] for k in blks] for c in range(self.nch)}
        if self.nch == 2:
            self.lines["mid"] = [k["lines"] for k in MR.mid_blocks(buf, n_short, blksw_bits)[1]]
        self._lo, self._B = {}, {}

    def column(self, mix, c=0):
        """what out channel c holds under mix (None: every channel; a mono file gives its own channel everywhere)"""
        if self.nch == 1:
            return 0
        return {None: c, "mid": "mid", "left": 0, "right": 1}[mix]

    def B(self, edges, col):
        key = (tuple(edges), col)
        if key not in self._B:
            rows = []
            for (p, a, b), lines in zip(self.blocks, self.lines[col]):
                if (a, b, key[0]) not in self._lo:
                    self._lo[(a, b, key[0])] = line_ranges(self.fs, a, b, edges)
                rows.append(band_sums(lines, self._lo[(a, b, key[0])]))
            self._B[key] = np.array(rows).reshape(len(self.blocks), len(edges) - 1)
            self._B[key].setflags(write=False)
        return self._B[key]

    def window(self, edges, start, n_frames, hop, mix=None, channels=None):
        """-> float64 [channels][n_bands][n_frames] as the call writes it, and the blocks it parses"""
        channels = (1 if mix is not None else self.nch) if channels is None else channels
        out, needed = [], []
        for c in range(channels):
            o, needed = frames(self.blocks, self.B(edges, self.column(mix, c)), self.L, start, n_frames, hop)
            out.append(o)
        return np.array(out), needed
