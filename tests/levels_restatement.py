"""
The block energies of mrc_pac_store_block_energy restated in NumPy from the decoded lines of tests/reduced_restatement.blocks
and tests/mix_restatement.mid_blocks -- e = ((a + b) / D) * sum(lines[:(a + b) // (2 D)] ** 2) -- and the oracle-side
constructions the levels tests share (tests/test_store_levels_cpu.py, tests/test_gpu_store_levels.py).  A plain module.

kernel_sum adds in block_energy_kernel's documented order (mrc_kernels_store.hip): lane l of 64 adds the squares of lines
l, l + 64, ... one after the other from +0.0, then a balanced tree over the lanes in their natural order.  With it the
restatement is the kernel's value to the bit; np.sum (pairwise) differs from it by rounding alone, at most
2 (n + 1) 2^-53 relative for n non-negative terms.
"""
import numpy as np

import mix_restatement as MR
import mono_oracle
import reduced_restatement as RR
import settings_kit as SK
from oracle import codec as ocodec, mdct as omdct, pacfile as opac
from oracle.window import TransitionWindow

WAVE = 64


def kernel_sum(sq):
    """the sum of the non-negative terms sq in block_energy_kernel's order"""
    lanes = np.zeros(WAVE)
    for l in range(min(WAVE, len(sq))):
        acc = 0.0
        for v in sq[l::WAVE]:
            acc = acc + v
        lanes[l] = acc
    while len(lanes) > 1:
        lanes = lanes[0::2] + lanes[1::2]
    return float(lanes[0])


def block_energies(buf, n_short, blksw_bits, D, mid=False, order="kernel"):
    """-> (nCh, blocks int64 [n][3] (start, a, b), energy float64 [n][nCh or 1], lines summed per block [n]);
    mid: the mid of a stereo file on the lines (mix_restatement), a mono file's own channel"""
    cp, blks = RR.blocks(buf, n_short, blksw_bits)
    nch = cp.nChannels
    if mid and nch == 2:
        _, mblks = MR.mid_blocks(buf, n_short, blksw_bits)
        rows = [[k["lines"]] for k in mblks]
    else:
        rows = [k["lines"] for k in blks]
    add = kernel_sum if order == "kernel" else (lambda sq: float(np.sum(sq)))
    blocks = np.array([(k["start"], k["a"], k["b"]) for k in blks], dtype=np.int64).reshape(-1, 3)
    energy = np.zeros((len(blks), len(rows[0]) if rows else 1))
    n_lines = np.zeros(len(blks), np.int64)
    for i, (k, row) in enumerate(zip(blks, rows)):
        N = k["a"] + k["b"]
        if N % (2 * D):
            raise ValueError("block shape (%d,%d) does not divide by %d" % (k["a"], k["b"], D))
        n_lines[i] = N // (2 * D)
        for c, lines in enumerate(row):
            x = np.asarray(lines, dtype=np.float64)[:n_lines[i]]
            energy[i, c] = (N // D) * add(x * x)
    return nch, blocks, energy, n_lines


# ------------------------------------------------------------------ oracle transforms only: what the estimate resolves
def block_sequence(n_hops, short, L, S):
    """hop h is one long block or, where short[h], L / S blocks of S new samples -> [(start, a, b)], a_0 = L, a_{i+1} = b_i"""
    bs = []
    for h in range(n_hops):
        bs += [S] * (L // S) if short[h] else [L]
    out, start, a = [], 0, L
    for b in bs:
        out.append((start, a, b))
        start += a
        a = b
    return out


def analyse(x, seq, L):
    """x [n] behind L zeros (the MDCT's delay), zeros behind it: the windowed MDCT lines of every block of seq, oracle code"""
    total = seq[-1][0] + seq[-1][1] + seq[-1][2]
    plane = np.zeros(total)
    plane[L:L + len(x)] = x[:total - L]
    return [omdct.MDCT(TransitionWindow(plane[p:p + a + b], a, b), a, b) for (p, a, b) in seq]


# ------------------------------------------------------------------ files whose whole energy lies inside [0, n_samples)
def silent_ends_file(n_channels, seed, L=1024, S=128, rate=48000):
    """a six-hop file of the default setting from the oracle's encoders whose first and last hop are digital silence --
    (L,L), (L,L), (L,S), (S,S).., (S,L), (L,L), (L,L) and Close()'s block; a tone over noise in hops 1 to 4 -- so that block 0
    decodes to zeros: nothing lies in the MDCT's delay, which decode_window drops"""
    cp = ocodec.default_params(sampleRate=rate, nChannels=n_channels, targetBitsPerSample=2.86)
    cp.nMDCTLines = cp.nSamplesPerBlock = cp.a = cp.b = L
    cp.nSamplesShort = S
    cp.sfBands = ocodec.bands_for_block(L, L, L, rate)
    cp.bitReservoir = 0
    ab = [(L, L)] * 2 + [(L, S)] + [(S, S)] * (L // S - 1) + [(S, L)] + [(L, L)] * 2
    offs = np.concatenate([[0], np.cumsum([a for a, _ in ab])[:-1]])
    n = 4 * L
    t = np.arange(n)
    tone = 0.25 * np.sin(2 * np.pi * 1000.0 / rate * t) + 0.075 * np.sin(2 * np.pi * 5200.0 / rate * t)
    x = tone[None] + 0.05 * np.random.default_rng(seed).standard_normal((n_channels, n))
    pcm = np.zeros((n_channels, 7 * L), np.int16)                    # the prior hop, a silent hop, four hops, a silent hop
    pcm[:, 2 * L:6 * L] = np.clip(np.rint(x * 32767.5), -32767, 32767).astype(np.int16)
    shapes = [(int(o), a, b) for o, (a, b) in zip(offs, ab)]
    if n_channels == 2:
        return opac.encode_stereo_stream(SK.to_float(pcm), shapes, cp, huffman=True)
    return mono_oracle.encode_mono_stream(SK.to_float(pcm), shapes, cp, huffman=True)
