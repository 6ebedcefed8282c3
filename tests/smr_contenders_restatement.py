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

The maskers, the node grid and the node error bound are those of tests/smr_paths_restatement.py (any block length); this
module adds the selection rule of the one instantiation that has it.

Used by tests/test_gpu_smr_contenders.py to ASSERT what each input exercises; it decides nothing about the codes.
"""
import numpy as np

from oracle import fast
import smr_paths_restatement as paths
from smr_paths_restatement import WAVE, NODE_C, NODE_H_MAX, NODE_MIN_MASKERS, NODE_TOL

HOP = 1024
CAPACITY = 64                    # kContCap
NODE_MAX_MASKERS = paths.CEILING[HOP]
FLOOR_GUARD = 1e-12 * (1.0 + 2.0 ** -30)        # (the kernel's test: just above kSplFloorGuard, see kFloorHi)
SHRINK = 1.0 - 2.0 ** -30                        # the margin on L and on the comparison (roundings, node tolerance)


def wave_chunks(w):
    return (w, 7 - w, 8 + w, 15 - w)


def analyse(block, scaled_lines, sample_rate=48000):
    """One long block [2048] and its scaled MDCT lines [1024] -> what the kernel's selection does with it."""
    M = HOP
    zb, quiet = paths.line_grid(M, sample_rate)
    mk = paths.maskers(block, sample_rate)
    P = mk["P"]
    a2 = 2. * (np.abs(scaled_lines) ** 2.) / (1. / 2.)
    out = dict(maskers=P, nodes=False, per_wave=[0] * 4, whole_chunks=set(), bound_fail_contenders=0, over_capacity=False,
               contenders=0)
    if P == 0:
        return out
    h, s0 = paths.node_grid(mk["slope"])
    out["nodes"] = bool(NODE_MIN_MASKERS <= P <= NODE_MAX_MASKERS and h <= NODE_H_MAX)
    if not out["nodes"]:
        return out
    nt = paths.node_terms(mk, zb, quiet, h, s0)
    n_up, t_lb, t = nt["n_up"], nt["t_lb"], nt["t"]
    row_ub = np.minimum(4 * ((n_up + NODE_C - 1) // NODE_C), P)
    t_ub = t_lb + nt["E0"] * nt["col_lam"][row_ub]
    assert np.all(t_ub >= t * (1 - 1e-12))
    bound_fails = ~(nt["bound"] <= NODE_TOL * t)
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
