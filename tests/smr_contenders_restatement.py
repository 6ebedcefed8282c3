"""
NumPy restatement of how the mono long-block smr_kernel chooses the lines it evaluates in full (csrc/mrc_smr_body.hpp, "band
contenders"), on the oracle's expressions: fast.masked_threshold_batch's masked intensity of a line split into its sides,

    t = quiet + in-band (|dz| <= 1/2) + lower side (dz < -1/2) + upper side (dz > 1/2),      dz = z_line - z_masker,

all positive.  t_lb = the first three.  t_ub = t_lb + E0 * sum over the maskers of the line's row of Lambda_m I_m 2^(-s0 z_m),
where s0 is the shallowest slope node, E0 = 2^(s0 (z_line - 1/2)), the row ends at the next multiple of four maskers at or
behind the line's upper-side count, and Lambda_m >= 1 is the sum of the absolute Lagrange weights of the masker's slope on
the 16 nodes.  A wave owns the 64-line chunks {w, 7 - w, 8 + w, 15 - w}; per band it takes L = max a2 / t_ub over its own
lines and keeps the lines with a2 >= L t_lb (both with a margin of 2^-30).  A chunk with a line whose a2 or t_lb is at the SPL floor guard is evaluated
whole; so is the chunk of a contender whose node error bound exceeds 1e-13 of its t, and every chunk of a wave with more
than 64 contenders.

Used by tests/test_gpu_smr_contenders.py to ASSERT what each input exercises; it decides nothing about the codes.
"""
import math

import numpy as np

from oracle import fast
from oracle.psychoac import Thresh, Bark, Intensity, SPL

HOP = 1024
WAVE = 64
CAPACITY = 64                    # kContCap
NODE_R, NODE_MARGIN, NODE_C = 16, 1, 4
NODE_H_MAX, NODE_H_MIN, NODE_MIN_MASKERS, NODE_MAX_MASKERS = 0.22, 1e-3, 32, 308
NODE_TOL, NODE_ROUND_EPS = 1e-13, 8.0 * 2.0 ** -53
FLOOR_GUARD = 1e-12 * (1.0 + 2.0 ** -30)        # (the kernel's test: just above kSplFloorGuard, see kFloorHi)
SHRINK = 1.0 - 2.0 ** -30                        # the margin on L and on the comparison (roundings, node tolerance)
LOG2_10 = math.log2(10.0)


def wave_chunks(w):
    return (w, 7 - w, 8 + w, 15 - w)


def _lagrange_abs(theta):
    """theta[P] -> (Lambda[P] = sum_r |lambda_r(theta)|, |prod_r (theta - r)| / R!)"""
    r = np.arange(NODE_R)
    d = theta[:, None] - r[None, :]                                  # [P, R]
    lam = np.empty_like(d)
    for j in range(NODE_R):
        others = np.delete(r, j)
        lam[:, j] = np.prod(d[:, others], axis=1) / np.prod(j - others)
    return np.abs(lam).sum(axis=1), np.abs(np.prod(d, axis=1)) / math.factorial(NODE_R)


def analyse(block, scaled_lines, sample_rate=48000):
    """One long block [2048] and its scaled MDCT lines [1024] -> what the kernel's selection does with it."""
    N, M = 2 * HOP, HOP
    n = np.arange(M)
    zb = Bark((n + 0.5) * ((float(sample_rate) / M) / 2.))
    quiet = Intensity(Thresh((n + 0.5) * ((float(sample_rate) / M) / 2.)))
    X = np.fft.fft(np.multiply(block, fast._hann(N)))
    XI = 4. * (np.abs(X) ** 2.) / ((N ** 2.) * (3. / 8.))
    last = N // 2 - 100
    c = XI[1:last - 1]
    p = np.nonzero((c > XI[0:last - 2]) & (c > XI[2:last]))[0] + 1
    P = len(p)
    a2 = 2. * (np.abs(scaled_lines) ** 2.) / (1. / 2.)
    out = dict(maskers=P, nodes=False, per_wave=[0] * 4, whole_chunks=set(), bound_fail_contenders=0, over_capacity=False,
               contenders=0)
    if P == 0:
        return out
    x0, x1, x2 = XI[p - 1], XI[p], XI[p + 1]
    s3 = (x0 + x1) + x2
    level = SPL(s3)
    f = fast.py2div(sample_rate, N) * (((p - 1) * x0 + p * x1) + (p + 1) * x2) / s3
    zm = Bark(f)
    boost = 0.37 * np.maximum(level - 40, 0)
    I = Intensity(level - 15.0)
    slope = ((-27 + boost) * 0.1) * LOG2_10                          # bits per Bark, upper side
    h = max((slope.max() - slope.min()) / (NODE_R - 1 - 2 * NODE_MARGIN), NODE_H_MIN)
    s0 = slope.max() + NODE_MARGIN * h
    out["nodes"] = bool(NODE_MIN_MASKERS <= P <= NODE_MAX_MASKERS and h <= NODE_H_MAX)
    if not out["nodes"]:
        return out
    assert np.all(np.diff(zm) >= 0), "maskers in bin order are in Bark order"
    dz = zb[:, None] - zm[None, :]                                   # [M, P]
    upper, lower, inband = dz > 0.5, dz < -0.5, np.abs(dz) <= 0.5
    n_up = upper.sum(axis=1)
    assert np.array_equal(upper, np.arange(P)[None, :] < n_up[:, None])
    t_lb = quiet + (inband * I).sum(axis=1) + (lower * I * np.power(2.0, (-2.7 * LOG2_10) * (np.abs(dz) - 0.5) * lower)).sum(axis=1)
    up = (upper * I * np.power(2.0, slope * (dz - 0.5) * upper)).sum(axis=1)
    t = t_lb + up
    Lam, err_prod = _lagrange_abs((s0 - slope) / h)
    zq = zb - 0.5
    E0 = np.power(2.0, s0 * zq)
    F0 = I * np.power(2.0, -s0 * zm)
    col_lam = np.concatenate([[0.0], np.cumsum(Lam * F0)])           # prefix sums over maskers
    col_err = np.concatenate([[0.0], np.cumsum(I * err_prod)])
    row_ub = np.minimum(4 * ((n_up + NODE_C - 1) // NODE_C), P)
    t_ub = t_lb + E0 * col_lam[row_ub]
    assert np.all(t_ub >= t * (1 - 1e-12))
    row = 4 * (n_up // NODE_C)
    xr = (h * NODE_R) / (-s0)
    psi = xr ** 16 * math.exp(-16.0)
    bound = psi * col_err[row] + (NODE_ROUND_EPS * E0) * col_lam[row]
    bound_fails = ~(bound <= NODE_TOL * t)
    band_of = np.empty(M, dtype=int)
    sfb = fast.bands_for(HOP, HOP)
    for b in range(sfb.nBands):
        band_of[sfb.lowerLine[b]:sfb.upperLine[b] + 1] = b
    for w in range(4):
        lines = []
        for ch in wave_chunks(w):
            sl = np.arange(ch * WAVE, (ch + 1) * WAVE)
            if np.any(~((a2[sl] >= FLOOR_GUARD) & (t_lb[sl] >= FLOOR_GUARD))):
                out["whole_chunks"].add(ch)
            else:
                lines.append(sl)
        if not lines:
            continue
        lines = np.concatenate(lines)
        keep = np.zeros(len(lines), dtype=bool)
        for b in np.unique(band_of[lines]):
            sel = band_of[lines] == b
            L = np.max(a2[lines[sel]] / t_ub[lines[sel]]) * SHRINK
            keep[sel] = ~(a2[lines[sel]] < (L * t_lb[lines[sel]]) * SHRINK)
            assert np.max(a2[lines[sel]] / t[lines[sel]]) == np.max((a2[lines] / t[lines])[sel & keep]), "a pruned line won"
        out["per_wave"][w] = int(keep.sum())
        if keep.sum() > CAPACITY:
            out["over_capacity"] = True
            out["whole_chunks"].update(wave_chunks(w))
        else:
            fails = lines[keep][bound_fails[lines[keep]]]
            out["bound_fail_contenders"] += len(fails)
            out["whole_chunks"].update(int(k) // WAVE for k in fails)
    out["contenders"] = int(sum(out["per_wave"]))
    out["median_ub_over_t"] = float(np.median(t_ub / t))
    return out


def analyse_blocks(blocks):
    """[B, 2048] -> list of analyse() results, with the oracle's own scaled lines"""
    blocks = np.asarray(blocks, dtype=np.float64)
    X = fast.mdct_batch(blocks, HOP, HOP)
    _, Xs = fast.overall_scale_batch(X, fast.DEFAULTS["nScaleBits"])
    return [analyse(blocks[i], Xs[i]) for i in range(len(blocks))]
