"""
NumPy account of which evaluation smr_kernel (csrc/mrc_smr_body.hpp, mrc_smr_sweep.hpp) chooses for ONE (block, signal) unit
of any block length N = a + b, on the oracle's expressions (fast.masked_threshold_batch's maskers and its masked intensity of
a line, split into its sides):

    t = quiet + in-band (|dz| <= 1/2) + lower side (dz < -1/2) + upper side (dz > 1/2),      dz = z_line - z_masker.

The kernel evaluates the upper side of a unit
  * through the slope nodes when the block length has them (CEILING), the unit has between NODE_MIN_MASKERS and its ceiling
    of maskers, and the range of their upper slopes fits 13 node spacings of at most NODE_H_MAX bit per Bark; a 64-line chunk
    with a line whose node error bound exceeds NODE_TOL of its masked intensity goes back to the sorted sweep;
  * by the sorted sweep for the whole unit otherwise ("slope": range too wide, "few", "many": masker count, "length": a block
    length whose instantiation has no nodes -- the short block and every length of a non-default handle);
  * not at all beyond the quiet threshold when the unit has no masker ("none").

The arithmetic of the maskers and of the node bound exists once, here; tests/smr_contenders_restatement.py (the mono long
block's band contenders) builds on it.  Used by tests/test_smr_paths_cpu.py and tests/test_gpu_smr_paths.py to ASSERT what each
input exercises; it decides nothing about the codes.
"""
import math

import numpy as np

from oracle import fast
from oracle.psychoac import Thresh, Bark, Intensity, SPL

WAVE = 64
# mrc_smr_sweep.hpp: kNodeR, kNodeMargin, kNodeC, kNodeHMax, kNodeHMin, kNodeMinMaskers, kNodeTol, kNodeRoundEps
NODE_R, NODE_MARGIN, NODE_C = 16, 1, 4
NODE_H_MAX, NODE_H_MIN, NODE_MIN_MASKERS = 0.22, 1e-3, 32
NODE_TOL, NODE_ROUND_EPS = 1e-13, 8.0 * 2.0 ** -53
LOG2_10 = math.log2(10.0)
# lines of the block (DIM) -> the most maskers a unit takes through the nodes.  mrc_smr_sweep.hpp:
#   "__host__ __device__ constexpr int node_max_maskers(int DIM)"   (static_assert(node_max_maskers(1024) == 308, ...));
# mrc_smr_body.hpp gives the nodes to DIM == 1024 and DIM == 576 only ("constexpr bool kNodes = (DIM == 1024 || DIM == 576)").
# node_max_maskers() below restates the header's function; tests/test_smr_paths_cpu.py holds the table against it.
CEILING = {1024: 308, 576: 156}
LOG_TAB_DOUBLES = 128                              # kLogTabEntries * 4 (mrc_log10.hpp)


def node_max_maskers(dim, log_len=LOG_TAB_DOUBLES):
    """mrc_smr_sweep.hpp, smr_layout(DIM, DIM, DIM - 100) and node_max_maskers(DIM), in integers"""
    H = M = dim
    last = dim - 100
    pk_shorts = (last // 2 + 5) & ~3
    pi_off = 2 * H + (pk_shorts * 2 + 2 * (M + 2) * 2) // 8
    pi_len = 2 * (last // 2 + 2)
    if pi_off + max(pi_len, M) + log_len <= 4 * H:
        log_off = 4 * H - log_len
    else:
        total = 4 * H + last + 1
        total += total & 1
        log_off = total + M
    q_start = 2 * dim + (2 * (dim + 2) * 2) // 8
    if log_off <= q_start or log_off >= 4 * dim:
        return 0
    rows = (log_off - q_start) // 18
    return max(min((rows - 1) * 4, (2 * dim - 96 - 2) // 6, 3 * 26 * 4 - 4), 0)


def max_peaks(N):
    """strict 3-point peaks at bins 1 .. N/2 - 102, no two adjacent (psychoac.py:160)"""
    return (N // 2 - 101) // 2


def line_grid(M, sample_rate=48000):
    """-> (Bark value, quiet-threshold intensity) of the M lines, as fast.masked_threshold_batch forms them"""
    f = (np.arange(M) + 0.5) * ((float(sample_rate) / M) / 2.)
    return Bark(f), Intensity(Thresh(f))


def maskers(block, sample_rate=48000):
    """One block [N] -> its tonal maskers in bin order: dict(P, zm, I, slope (upper side, bit per Bark))"""
    N = len(block)
    X = np.fft.fft(np.multiply(block, fast._hann(N)))
    XI = 4. * (np.abs(X) ** 2.) / ((N ** 2.) * (3. / 8.))
    last = N // 2 - 100
    c = XI[1:last - 1]
    p = np.nonzero((c > XI[0:last - 2]) & (c > XI[2:last]))[0] + 1
    if len(p) == 0:
        return dict(P=0)
    x0, x1, x2 = XI[p - 1], XI[p], XI[p + 1]
    s3 = (x0 + x1) + x2
    level = SPL(s3)
    f = fast.py2div(sample_rate, N) * (((p - 1) * x0 + p * x1) + (p + 1) * x2) / s3
    zm = Bark(f)
    boost = 0.37 * np.maximum(level - 40, 0)
    I = Intensity(level - 15.0)
    slope = ((-27 + boost) * 0.1) * LOG2_10                          # bits per Bark, upper side
    return dict(P=len(p), zm=zm, I=I, slope=slope)


def node_grid(slope):
    """the unit's node spacing and shallowest node (bit per Bark): 13 spacings over its slope range, a margin on either side"""
    h = max((slope.max() - slope.min()) / (NODE_R - 1 - 2 * NODE_MARGIN), NODE_H_MIN)
    return h, slope.max() + NODE_MARGIN * h


def _lagrange_abs(theta):
    """theta[P] -> (Lambda[P] = sum_r |lambda_r(theta)|, |prod_r (theta - r)| / R!)"""
    r = np.arange(NODE_R)
    d = theta[:, None] - r[None, :]                                  # [P, R]
    lam = np.empty_like(d)
    for j in range(NODE_R):
        others = np.delete(r, j)
        lam[:, j] = np.prod(d[:, others], axis=1) / np.prod(j - others)
    return np.abs(lam).sum(axis=1), np.abs(np.prod(d, axis=1)) / math.factorial(NODE_R)


def node_terms(mk, zb, quiet, h, s0):
    """The sides of every line's masked intensity and the node evaluation's error bound per line.
    -> dict(n_up, t_lb, t, E0, col_lam, col_err, bound): col_* are prefix sums over the maskers ([P + 1]); the bound is taken
    at the line's row (every fourth masker, NODE_C) as the kernel takes it."""
    zm, I, slope, P = mk["zm"], mk["I"], mk["slope"], mk["P"]
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
    row = NODE_C * (n_up // NODE_C)
    xr = (h * NODE_R) / (-s0)
    psi = xr ** 16 * math.exp(-16.0)
    bound = psi * col_err[row] + (NODE_ROUND_EPS * E0) * col_lam[row]
    return dict(n_up=n_up, t_lb=t_lb, t=t, E0=E0, col_lam=col_lam, col_err=col_err, bound=bound)


def account(block, sample_rate=48000):
    """One block [N] of one signal -> what the kernel does with the unit:
      maskers      their count
      nodes, why   True, None -- or False and "slope" | "few" | "many" | "none" | "length"
      chunk_ratio  per 64-line chunk the largest bound / (NODE_TOL t) of its lines (nodes only, else empty)
      chunks       the chunks where that exceeds 1: sent back to the sorted sweep
      ratio        the largest of chunk_ratio (0 without nodes)"""
    block = np.asarray(block, dtype=np.float64)
    M = len(block) // 2
    mk = maskers(block, sample_rate)
    P = mk["P"]
    out = dict(maskers=P, nodes=False, why=None, chunk_ratio=np.zeros(0), chunks=set(), ratio=0.0)
    if P == 0:
        out["why"] = "none"
        return out
    if M not in CEILING:
        out["why"] = "length"
        return out
    h, s0 = node_grid(mk["slope"])
    if P < NODE_MIN_MASKERS:
        out["why"] = "few"
    elif P > CEILING[M]:
        out["why"] = "many"
    elif not h <= NODE_H_MAX:
        out["why"] = "slope"
    if out["why"]:
        return out
    zb, quiet = line_grid(M, sample_rate)
    nt = node_terms(mk, zb, quiet, h, s0)
    r = nt["bound"] / (NODE_TOL * nt["t"])
    n_chunks = (M + WAVE - 1) // WAVE
    cr = np.array([r[c * WAVE:(c + 1) * WAVE].max() for c in range(n_chunks)])
    out.update(nodes=True, chunk_ratio=cr, chunks=set(int(c) for c in np.nonzero(~(cr <= 1.0))[0]), ratio=float(cr.max()))
    return out


def needed_chunks(switch_row, sig, sfb, M):
    """Joint stereo: the 64-line chunks of signal `sig` (0 L, 1 R, 2 M, 3 S) with a line in a band whose SMR the encoder takes
    from this signal (ms_stereo.py:70-81); the kernel skips the others.  An all-False answer: the unit is not evaluated."""
    want = (np.asarray(switch_row) != 0) == (sig >= 2)
    on_line = np.repeat(want, sfb.nLines)[:M]
    n_chunks = (M + WAVE - 1) // WAVE
    return np.array([on_line[c * WAVE:(c + 1) * WAVE].any() for c in range(n_chunks)])


CLEAN_BELOW, SENT_FROM = 0.5, 4.0          # bound / (tol t): clearly nothing sent back / clearly a chunk sent back


def classify(acc):
    """the class of an evaluated unit's account (with `needed`): "clean" (nodes, no needed chunk near the tolerance), "sent"
    (nodes, a needed chunk at SENT_FROM x tol or more), the reason of a whole-unit sorted sweep, or None (nodes, in between)"""
    if not acc["nodes"]:
        return acc["why"]
    r = acc["chunk_ratio"][acc["needed"]].max()
    return "clean" if r <= CLEAN_BELOW else "sent" if r >= SENT_FROM else None


def sent_chunks(acc, factor=SENT_FROM):
    """needed chunks of a unit through the nodes whose bound is at least factor x tol"""
    return int((acc["chunk_ratio"][acc["needed"]] >= factor).sum()) if acc["nodes"] else 0


def joint_accounts(left, right, a, b, n_mdct_lines=1024, sample_rate=48000):
    """Blocks [B][a + b] of both channels -> (the oracle's ms_switch [B][nBands], accounts [B][4]) for the signals L, R, M, S as the
    oracle forms them; every account carries `needed` (its chunks the kernel does not skip) and `evaluated` (any of them)."""
    sfb = fast.bands_for(a, b, n_mdct_lines, sample_rate)
    sw = fast.ms_switch_batch(fast.mdct_batch(left, a, b), fast.mdct_batch(right, a, b), sfb)
    sigs = [left, right, (left + right) / 2.0, (left - right) / 2.0]
    out = []
    for f in range(len(left)):
        row = []
        for s in range(4):
            acc = account(sigs[s][f], sample_rate)
            acc["needed"] = needed_chunks(sw[f], s, sfb, (a + b) // 2)
            acc["evaluated"] = bool(acc["needed"].any())
            row.append(acc)
        out.append(row)
    return sw, out
