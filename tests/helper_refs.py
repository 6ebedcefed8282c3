"""
References and input sets for the probes of the kernels' __device__ helpers (csrc/mrc_kernels_probe.hip,
tests/test_gpu_helper_probes.py; the references themselves are held by tests/test_helper_refs_cpu.py).

  * NumPy LANE MODELS of the cross-lane moves (csrc/mrc_wave.hpp): which lane every lane reads, as the comments there state
    it, and the reductions, folds and the scan composed of them exactly as the header composes them.  Arrays are [..., 64].
  * exact references of the math helpers: np.longdouble (64-bit mantissa, 11 bits beyond a double) over whole input sets, and
    mpmath / fractions at 80 digits for the elements that come out worst -- the figure a test asserts is the 80-digit one.
  * an exact restatement of the quantiser (quantize.py:12-38, 114-146, 294-322 of the reference) in which every floating-point
    operation is one correctly rounded Fraction -> float conversion.
  * the input sets, each at most 2^16 elements, with the edge classes named in their docstrings (asserted on the CPU).

Errors in ulps are in ulps of the EXACT value: |got - exact| / 2^(floor(log2 |exact|) - 52).
"""
import os
import re
from fractions import Fraction

import mpmath
import numpy as np

mpmath.mp.dps = 80
LD = np.longdouble
LANE = np.arange(64)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mrcaudiocodec_amd", "csrc")
MAX_SET = 1 << 16


# ------------------------------------------------------------------------------------------------ lane models (mrc_wave.hpp)
# lane i reads the lane the DPP control names: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror (the other quad of
# the 8-lane group, mirrored), row_ror:8 (the other half of the 16-lane row)
DPP_SOURCE = {0xB1: LANE ^ 1, 0x4E: LANE ^ 2, 0x141: LANE ^ 7, 0x128: LANE ^ 8}


def dpp_move(ctrl, v):
    return np.asarray(v)[..., DPP_SOURCE[ctrl]]


def rows_swap(dist, a, b):
    """x: both registers' even rows / lower half (a's where they were, b's in the odd rows / upper half); y: both registers'
    odd rows / upper half (b's where they were, a's in the even rows / lower half)"""
    a, b = np.asarray(a), np.asarray(b)
    upper = (LANE & dist) != 0
    x = np.where(upper, b[..., (LANE - dist) % 64], a)
    y = np.where(upper, b, a[..., (LANE + dist) % 64])
    return x, y


def rows_combine(dist, v, op):
    x, y = rows_swap(dist, v, v)
    return op(x, y)


def row_reduce(v, op):
    for ctrl in (0xB1, 0x4E, 0x141, 0x128):
        v = op(v, dpp_move(ctrl, v))
    return v


def wave_allreduce(v, op):
    v = row_reduce(v, op)
    v = rows_combine(16, v, op)
    return rows_combine(32, v, op)


def wave_fold4(a, b, c, d, op):
    x, y = rows_swap(32, a, c)
    ac = op(x, y)
    x, y = rows_swap(32, b, d)
    bd = op(x, y)
    x, y = rows_swap(16, ac, bd)
    return row_reduce(op(x, y), op)


def wave_fold2(a, b, op):
    x, y = rows_swap(32, a, b)
    return rows_combine(16, row_reduce(op(x, y), op), op)


def row_shr(k, v):
    """row_shr:k with bound_ctrl: lane i of a row reads lane i - k of the same row, 0 where there is none"""
    v = np.asarray(v)
    return np.where((LANE & 15) >= k, v[..., (LANE - k) % 64], np.zeros_like(v))


def row_bcast(last, rows, v):
    """row_bcast:15 / row_bcast:31 under a row mask: the lanes of the rows in `rows` read lane `last` of the row (15) or of
    the half (31) BEFORE theirs; the other rows keep the prepared zero"""
    v = np.asarray(v)
    src = ((LANE // (last + 1)) * (last + 1) - 1) % 64
    return np.where(np.isin(LANE // 16, rows), v[..., src], np.zeros_like(v))


def wave_incl_scan(v):
    v = np.asarray(v)
    for k in (1, 2, 4, 8):
        v = v + row_shr(k, v)
    v = v + row_bcast(15, (1, 3), v)
    return v + row_bcast(31, (2, 3), v)


def wave_sum_block8(v):
    """mrc_smr_math.hpp: wave_sum_block<8>; v [..., 8, 64] -> [..., 8, 64] (every lane ends with all eight totals)"""
    v = np.asarray(v)
    add = lambda p, q: sum(rows_swap(p, v[..., q[0], :], v[..., q[1], :]))
    a = [add(32, (k, k + 4)) for k in range(4)]
    b0 = sum(rows_swap(16, a[0], a[2]))
    b1 = sum(rows_swap(16, a[1], a[3]))
    s0 = b0 + dpp_move(0x128, b0)
    s1 = b1 + dpp_move(0x128, b1)
    s = np.where((LANE & 8) != 0, s1, s0)
    for ctrl in (0xB1, 0x4E, 0x141):
        s = s + dpp_move(ctrl, s)
    return np.stack([np.broadcast_to(s[..., 8 * j:8 * j + 1], s.shape) for j in range(8)], axis=-2)


# ------------------------------------------------------------------------------------------------ wave input sets
N_WAVES = 72            # a multiple of 1, 3, 4 and 12 waves per launch (64 / 256 threads, 1 / 3 workgroups); >= 64 for "each lane"


def wave_tags():
    """lane + 64 * wave"""
    return (LANE[None, :] + 64 * np.arange(N_WAVES)[:, None]).astype(np.int64)


def exact_sum_doubles(seed, shape=(N_WAVES, 64)):
    """integer-valued doubles, |v| < 2^20: every order of 64 (or 64 x 17) additions is exact"""
    return np.random.default_rng(seed).integers(-(1 << 20), 1 << 20, size=shape).astype(np.float64)


def exact_sum_ints(seed, shape=(N_WAVES, 64)):
    return np.random.default_rng(seed).integers(-(1 << 20), 1 << 20, size=shape).astype(np.int64)


def max_permutations(seed):
    """[N_WAVES][64] doubles: per wave a permutation of 64 distinct values, 40 of them negative, with the maximum in lane
    `wave` for the first 64 waves"""
    rng = np.random.default_rng(seed)
    out = np.empty((N_WAVES, 64))
    base = (np.arange(64) - 40) * 1.5 + 0.25
    for w in range(N_WAVES):
        p = rng.permutation(base)
        at = int(np.argmax(p))
        p[[at, w % 64]] = p[[w % 64, at]]
        out[w] = p
    return out


def all_negative_permutations(seed):
    """as max_permutations with every value negative (a reduction that starts from 0 would show)"""
    return max_permutations(seed) - 100.0


def signed_zero_waves():
    """[N_WAVES][64]: -0.0 everywhere with one +0.0 in lane `wave` (first 64 waves); then all -0.0, all +0.0, and waves whose
    maximum is -0.0 over negative values"""
    out = np.full((N_WAVES, 64), -0.0)
    for w in range(64):
        out[w, w] = 0.0
    out[65] = 0.0
    for w in range(66, N_WAVES):
        out[w] = -1.0 - LANE
        out[w, (7 * w) % 64] = -0.0
    return out


def scan_steps():
    """[N_WAVES][64] ints: a single 1 at lane `wave` (first 64 waves), then all ones and zeros"""
    out = np.zeros((N_WAVES, 64), dtype=np.int64)
    for w in range(64):
        out[w, w] = 1
    out[64:68] = 1
    return out


def ordered_doubles():
    """a strictly increasing list: -inf, large negatives, negative denormals, -0.0, +0.0, positive denormals, values around 1,
    DBL_MAX, +inf"""
    tiny, big = 5e-324, 1.7976931348623157e308
    one = [np.nextafter(1.0, 0.0), 1.0, np.nextafter(1.0, 2.0)]
    pos = [tiny, 2 * tiny, 1e-310, 2.2250738585072009e-308, 2.2250738585072014e-308, 1e-300, 1e-12, 0.5] + one + \
          [2.0, 1e12, 1e300, np.nextafter(big, 0.0), big]
    neg = [-v for v in reversed(pos)]
    return np.array([-np.inf] + neg + [-0.0, 0.0] + pos + [np.inf], dtype=np.float64)


XCD_GRIDS = (1, 7, 8, 9, 63, 64, 65, 1000, 3071, 3072, 3073)


def xcd_inputs():
    b = np.concatenate([np.arange(g) for g in XCD_GRIDS]).astype(np.int64)
    g = np.concatenate([np.full(g, g) for g in XCD_GRIDS]).astype(np.int64)
    return b, g


# ------------------------------------------------------------------------------------------------ errors
def ulp_of(exact):
    """2^(floor(log2 |exact|) - 52), as a long double"""
    _, e = np.frexp(np.abs(np.asarray(exact, dtype=LD)))
    return np.ldexp(LD(1), e - 53)


def ulp_err_ld(got, exact):
    return np.abs(np.asarray(got, dtype=LD) - exact) / ulp_of(exact)


def rel_err_ld(got, exact):
    return np.abs(np.asarray(got, dtype=LD) - exact) / np.abs(exact)


def mp_of(x):
    return mpmath.mpf(float(x))


def ulp_err_mp(got, exact):
    exact = mpmath.mpf(exact)
    return abs(mp_of(got) - exact) / mpmath.ldexp(1, int(mpmath.floor(mpmath.log(abs(exact), 2))) - 52)


def rel_err_mp(got, exact):
    exact = mpmath.mpf(exact)
    return abs(mp_of(got) - exact) / abs(exact)


def worst_case(err_ld, exact_mp_of_index, got, kind, keep=24):
    """The maximum of an error over a set: the long-double figures pick the `keep` worst elements, 80-digit arithmetic
    measures those (the long double reference is itself good to 2^-11 ulp of a double, far less than the gaps between the
    candidates).  Returns (maximum at 80 digits, its index, largest disagreement between the two figures on the candidates)."""
    err_ld = np.asarray(err_ld)
    idx = np.argsort(err_ld)[-keep:]
    f = ulp_err_mp if kind == "ulp" else rel_err_mp
    errs = [f(got[i], exact_mp_of_index(int(i))) for i in idx]
    k = int(np.argmax([float(e) for e in errs]))
    gap = max(abs(float(e) - float(err_ld[i])) for e, i in zip(errs, idx))
    return float(errs[k]), int(idx[k]), gap


# ------------------------------------------------------------------------------------------------ reciprocal
# What t_ub of the bound pass (mrc_smr_body.hpp) can hold: a chunk with a line whose t_lb is below kFloorHi = kSplFloorGuard
# (1 + 2^-30), just above 1e-12, never reaches the reciprocal, and t_ub >= t_lb, so the smallest exponent is that of 1e-12 (2^-40);
# upwards the sum of a frame's masker intensities, each 10^((SPL - 96) / 10) of at most 3 x 1024^2 x full scale -- taken to
# 2^64 (289 dB), far beyond it.
RCP_EXP_LO, RCP_EXP_HI = -40, 64


def _mantissas(n_even, n_random, seed):
    even = 1.0 + np.arange(n_even) / n_even
    rnd = 1.0 + np.random.default_rng(seed).random(n_random)
    lo = [1.0]
    for _ in range(3):
        lo.append(np.nextafter(lo[-1], 2.0))
    hi = [np.nextafter(2.0, 1.0)]
    for _ in range(3):
        hi.append(np.nextafter(hi[-1], 1.0))
    return np.concatenate([even, rnd, lo, hi])


def rcp_inputs():
    """positive normal doubles: 2^12 evenly spaced mantissas, 2^10 random ones and the four nearest either end of the binade at
    the exponents of 1e-12, 1 and 2^34 and at both extremes of the normal range (-1022, 1023); 64 + 64 + 8 mantissas at EVERY
    exponent t_ub can hold (RCP_EXP_LO .. RCP_EXP_HI) and at every 32nd exponent of the whole normal range"""
    full, small = _mantissas(1 << 12, 1 << 10, 11), _mantissas(64, 64, 12)
    exps_full = [RCP_EXP_LO, 0, 34, -1022, 1023]
    exps_small = sorted(set(range(RCP_EXP_LO, RCP_EXP_HI + 1)) | set(range(-1022, 1024, 32)))
    x = [np.ldexp(full, e) for e in exps_full] + [np.ldexp(small, e) for e in exps_small]
    return np.concatenate(x)


def line_ratio_inputs():
    """(a2, t): a2 = 0, 1e-30 .. 1e30 against t from 1e-12 to 1e20, and every a2 against t = +inf"""
    rng = np.random.default_rng(13)
    a2 = np.concatenate([[0.0], 10.0 ** rng.uniform(-30, 30, 4095)])
    t = 10.0 ** rng.uniform(-12, 20, 4096)
    return np.concatenate([a2, a2]), np.concatenate([t, np.full(4096, np.inf)])


# ------------------------------------------------------------------------------------------------ 2^x
def exp2_poly_inputs():
    """the ends of [-0.5, 0.5], 0, and 2^16 - 3 evenly spaced points"""
    return np.concatenate([[-0.5, 0.5, 0.0], np.linspace(-0.5, 0.5, MAX_SET - 3)])


def two_prod(a, b):
    """a * b = p + e exactly (Dekker; no overflow or underflow at the magnitudes used here)"""
    p = a * b
    split = 134217729.0
    ca, cb = split * a, split * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def exp2_tab_exact_ld(sT, u, T):
    """2^(sT u / T) of the EXACT product as a long double: sT u = n + g with n an integer and |g| <= 1/2 (exactly, from the
    two-product), n = T k + j, 2^((j + g) / T) 2^k -- an argument in [-1/2T, 1) keeps exp2l's error at 2^-64"""
    p, e = two_prod(np.asarray(sT, dtype=np.float64), np.asarray(u, dtype=np.float64))
    n = np.rint(p)
    g = (p - n).astype(LD) + e.astype(LD)
    n = n.astype(np.int64)
    k, j = n // T, n % T
    return np.ldexp(np.exp2((j.astype(LD) + g) / T), k.astype(np.int64)), g


def exp2_tab_exact_mp(sT, u, T):
    return mpmath.power(2, mp_of(sT) * mp_of(u) / T)


def exp2_tab_inputs():
    """(sT, u) with |sT u| < 16000: slopes in 1/64 .. 1/256 bit per Bark against Bark distances, zero products (sT = 0 and
    u = 0), products that are exact integers, exact half-integers (the rint tie) and the doubles either side of both"""
    rng = np.random.default_rng(17)
    sT = rng.uniform(-640.0, 640.0, 40000)
    u = rng.uniform(-25.0, 25.0, 40000)
    parts = [(sT, u), (np.zeros(64), rng.uniform(-25, 25, 64)), (rng.uniform(-640, 640, 64), np.zeros(64))]
    # exact integers and half-integers: sT a multiple of 1/8 below 2^10, u = m / sT is not exact -- take u a small integer
    # (or integer + 1/2 against an even multiple) so that the product is exact by construction
    a = rng.integers(-5000, 5000, 2048) / 8.0
    m = rng.integers(-24, 25, 2048).astype(np.float64)
    parts.append((a, m))                                            # multiples of 1/8: integers, halves, eighths
    a_int = rng.integers(-600, 600, 2048).astype(np.float64)
    parts.append((a_int, m))                                        # exact integers
    a_odd = (2 * rng.integers(-300, 300, 2048) + 1).astype(np.float64)
    h = m + 0.5
    parts.append((a_odd, h))                                        # odd x (m + 1/2): exact half-integers, the rint tie
    for s, v in ((a_int, m), (a_odd, h)):
        nz = v != 0
        parts.append((s[nz], np.nextafter(v[nz], np.inf)))          # ... and just beside them
        parts.append((s[nz], np.nextafter(v[nz], -np.inf)))
    sT = np.concatenate([p[0] for p in parts])
    u = np.concatenate([p[1] for p in parts])
    keep = np.abs(sT * u) < 15999.0
    return sT[keep][:MAX_SET], u[keep][:MAX_SET]


def exp2_dd_inputs():
    """(hi, lo): |hi| < 1000, |lo| < 2^-40; random, integers, half-integers (lo pointing back inside [-1/2, 1/2], the interval
    exp2_poly's claim is made on), and lo = 0"""
    rng = np.random.default_rng(19)
    hi = rng.uniform(-999.0, 999.0, 20000)
    lo = rng.uniform(-1.0, 1.0, 20000) * 2.0 ** -41
    k = rng.integers(-999, 999, 2048).astype(np.float64)
    lo_k = rng.uniform(-1.0, 1.0, 2048) * 2.0 ** -41
    halves = k + 0.5                                               # hi - rint(hi) = +-1/2 (ties to even)
    frac = halves - np.rint(halves)
    lo_h = -np.sign(frac) * np.abs(lo_k)
    return (np.concatenate([hi, k, halves, hi[:2048]]), np.concatenate([lo, lo_k, lo_h, np.zeros(2048)]))


# ------------------------------------------------------------------------------------------------ tables
def exp2_table(T):
    """2^(j/T), j < T, correctly rounded (80 digits, one rounding to double)"""
    return np.array([float(mpmath.power(2, mpmath.mpf(j) / T)) for j in range(T)])


def atan_q_fit(deg=21):
    """kAtanQ as tools/make_atan_poly.py defines it: the interpolant of atan(sqrt u) / sqrt u at the deg + 1 Chebyshev nodes
    of [0, 1], as monomials in u, each coefficient rounded once"""
    mp = mpmath.mp
    n = deg + 1
    g = lambda u: mpmath.mpf(1) if u == 0 else mpmath.atan(mpmath.sqrt(u)) / mpmath.sqrt(u)
    nodes = [mpmath.cos(mp.pi * (2 * j + 1) / (2 * n)) for j in range(n)]
    vals = [g((x + 1) / 2) for x in nodes]
    cheb = [sum(vals[j] * mpmath.cos(mp.pi * k * (2 * j + 1) / (2 * n)) for j in range(n)) * 2 / n for k in range(n)]
    cheb[0] /= 2
    T = [[mpmath.mpf(1)], [mpmath.mpf(0), mpmath.mpf(1)]]
    for k in range(2, n):
        a = [mpmath.mpf(0)] + [2 * c for c in T[k - 1]]
        b = T[k - 2] + [mpmath.mpf(0)] * (len(a) - len(T[k - 2]))
        T.append([x - y for x, y in zip(a, b)])
    px = [mpmath.mpf(0)] * n
    for k in range(n):
        for i, c in enumerate(T[k]):
            px[i] += cheb[k] * c
    q = [mpmath.mpf(0)] * n
    pw = [mpmath.mpf(1)]
    for i in range(n):
        for j, c in enumerate(pw):
            q[j] += px[i] * c
        nxt = [mpmath.mpf(0)] * (len(pw) + 1)
        for j, c in enumerate(pw):
            nxt[j] -= c
            nxt[j + 1] += 2 * c
        pw = nxt
    return np.array([float(c) for c in q])


def header_doubles(header, name):
    """the hexadecimal doubles of the initialiser of array `name` in csrc/<header>"""
    text = open(os.path.join(CSRC, header)).read()
    body = re.search(re.escape(name) + r"\[[^\]]*\](?:\[[^\]]*\])?\s*=\s*\{(.*?)\};", text, flags=re.S).group(1)
    return np.array([float.fromhex(t) for t in re.findall(r"-?0x[0-9a-fA-F.]+p[+-]?\d+", body)])


def log_table_words():
    """the log10 table as kLogTabDev lays it out for LDS: [j][4] = {1/c, log10 c hi, lo, 0}"""
    t = header_doubles("mrc_log10.hpp", "kLog10Tab").reshape(32, 3)
    return np.concatenate([t, np.zeros((32, 1))], axis=1).reshape(-1)


# ------------------------------------------------------------------------------------------------ double-double sums
def dd_inputs():
    """((hi, lo), (xh, xl)) double-doubles (|lo| <= ulp(hi) / 2): random pairs of one sign (what the prefix sums add), pairs
    far apart in magnitude (2^-60 .. 2^-200 of the first), and cancelling pairs: xh within a few ulps of -hi, the exact negative,
    and xh = -hi r with r in [1/2, 2] (the leading bits cancel, the low parts do not line up).  kinds: 0 one sign, 1 far apart,
    2 near negatives, 3 exact negatives, 4 partial cancellation"""
    rng = np.random.default_rng(23)

    def dd(h):
        l = np.ldexp(rng.uniform(-0.5, 0.5, h.shape), np.frexp(h)[1] - 53)       # |lo| <= ulp(hi) / 2
        s = h + l
        return s, l - (s - h)                                                    # (renormalised; exact here)
    n = 4096
    h1 = 10.0 ** rng.uniform(-12, 12, n)
    same = (dd(h1), dd(10.0 ** rng.uniform(-12, 12, n)))
    far = (dd(h1), dd(h1 * 2.0 ** -rng.integers(60, 200, n).astype(np.float64)))
    a = dd(h1)
    steps = rng.integers(-4, 5, n)
    xh = -a[0]
    for _ in range(4):
        xh = np.where(steps > 0, np.nextafter(xh, np.inf), np.where(steps < 0, np.nextafter(xh, -np.inf), xh))
        steps = steps - np.sign(steps)
    cancel = (a, dd(xh))
    exact_cancel = (a, (-a[0], -a[1]))
    partial = (a, dd(-a[0] * rng.uniform(0.5, 2.0, n)))
    cat = lambda k, m: np.concatenate([c[k][m] for c in (same, far, cancel, exact_cancel, partial)])
    kinds = np.repeat(np.arange(5), n)
    return (cat(0, 0), cat(0, 1)), (cat(1, 0), cat(1, 1)), kinds


def dd_exact(hi, lo, xh, xl):
    return [Fraction(float(a)) + Fraction(float(b)) + Fraction(float(c)) + Fraction(float(d))
            for a, b, c, d in zip(hi, lo, xh, xl)]


# ------------------------------------------------------------------------------------------------ atan, SPL
def atan_inputs():
    """x >= 0: 0, denormals, 2^16 - 2^12 points over [0, 1], the eight doubles either side of 1, and (1, 200]: the arguments
    0.00076 f and (f / 7500)^2 up to 96 kHz"""
    rng = np.random.default_rng(29)
    around = [1.0]
    for _ in range(4):
        around.append(np.nextafter(around[-1], 2.0))
    below = [np.nextafter(1.0, 0.0)]
    for _ in range(3):
        below.append(np.nextafter(below[-1], 0.0))
    head = np.array([0.0, 5e-324, 1e-310, 2.2250738585072014e-308] + below + around)
    unit = np.linspace(0.0, 1.0, MAX_SET - (1 << 12))
    big = np.concatenate([1.0 + 10.0 ** rng.uniform(-6, 0, 1024), rng.uniform(1.0, 200.0, (1 << 12) - 1024 - len(head) - 1),
                          [200.0]])
    return np.concatenate([head, unit, big])


def log10_inputs():
    """the argument classes of tests/log10_check.cpp (tests/test_abi.py::test_table_log10_accuracy): 10^U(-300, 300),
    1 + U(-0.01, 0.01) and 1 + 0.001 U(-0.01, 0.01)"""
    rng = np.random.default_rng(31)
    wide = 10.0 ** rng.uniform(-300, 300, 1 << 15)
    near = 1.0 + rng.uniform(-0.01, 0.01, 1 << 14)
    nearer = 1.0 + 0.001 * rng.uniform(-0.01, 0.01, 1 << 14)
    return np.concatenate([wide, near, nearer])


SPL_EDGES = np.array([0.0, 5e-324, 1e-310, -1.0, -np.inf, np.nan, np.inf, 2.2250738585072014e-308, -0.0])


# ------------------------------------------------------------------------------------------------ quantiser
def fl(q):
    """one rounding: the double nearest the rational q (ties to even)"""
    return float(Fraction(q))


def mag_code_exact(mag, n_bits):
    """quantize.py:12-38 for |x| = mag: 2^(R-1) - 1 from 1.0 on, else trunc(fl(fl(fl(2^R - 1) mag + 1) / 2)) -- three operations,
    three roundings (the division by two is exact)"""
    if mag >= 1.0:
        return (1 << (n_bits - 1)) - 1
    p = fl(Fraction((1 << n_bits) - 1) * Fraction(mag))
    s = fl(Fraction(p) + 1)
    return int(Fraction(s) / 2)


def scale_factor_exact(v, n_scale_bits, n_mant_bits):
    """quantize.py:114-146: leading zeros of the magnitude code below its top bit, capped at 2^Rs - 1"""
    cap = (1 << n_scale_bits) - 1
    n_bits = cap + n_mant_bits
    code = mag_code_exact(abs(v), n_bits)
    top = code.bit_length() - 1 if code > 0 else 0
    return min((n_bits - 2) - top, cap)


def mantissa_exact(x, scale, n_scale_bits, n_mant_bits):
    """quantize.py:294-322 for one element: sign bit at nMantBits - 1, the code shifted down by cap - scale"""
    cap = (1 << n_scale_bits) - 1
    code = mag_code_exact(abs(x), cap + n_mant_bits)
    return ((1 << (n_mant_bits - 1)) if x < 0.0 else 0) + (code >> max(cap - scale, 0))


def code_edge(c, n_bits):
    """the magnitude at which the code turns from c - 1 to c in exact arithmetic: ((2^R - 1) m + 1) / 2 = c"""
    return Fraction(2 * c - 1, (1 << n_bits) - 1)


def edge_codes(n_bits):
    """the codes whose lower edges are probed: 1 (the smallest magnitude with a non-zero code), 2, 3, every power of two (where
    the scale factor steps) and the code below it, the top code, and a few in between"""
    top = (1 << (n_bits - 1)) - 1
    cs = {1, 2, 3, top, top - 1, top // 3 + 1, (top * 5) // 7 + 1}
    for k in range(1, n_bits - 1):
        cs |= {1 << k, (1 << k) + 1}
    return sorted(c for c in cs if 1 <= c <= top)


def edge_magnitudes(n_bits):
    """per probed code: the double nearest its rational edge and the two doubles either side of it; then 0, the double just
    below 1.0 and 1.0 itself"""
    out = []
    for c in edge_codes(n_bits):
        m = fl(code_edge(c, n_bits))
        lo1 = np.nextafter(m, 0.0)
        hi1 = np.nextafter(m, 2.0)
        out += [np.nextafter(lo1, 0.0), lo1, m, hi1, np.nextafter(hi1, 2.0)]
    return np.array([v for v in out if 0.0 <= v < 1.0] + [0.0, np.nextafter(1.0, 0.0), 1.0])


N_BITS_ALL = tuple(range(2, 32))


def mag_code_inputs():
    mags = [edge_magnitudes(r) for r in N_BITS_ALL]
    return np.concatenate(mags), np.concatenate([np.full(len(m), r) for m, r in zip(mags, N_BITS_ALL)]).astype(np.int64)


def scale_mant_inputs():
    """x (both signs), scale, nScaleBits, nMantBits: every scale 0 .. cap for nScaleBits 1..4 and nMantBits 2..16, at a subset
    of the code width's edge magnitudes (the first code, a power of two, the top) and 0, 1 - ulp, 1"""
    xs, sc, sb, mb = [], [], [], []
    for s in range(1, 5):
        cap = (1 << s) - 1
        for m in range(2, 17):
            r = cap + m
            top = (1 << (r - 1)) - 1
            mags = []
            for c in sorted({1, 2, 1 << (r // 2), (1 << (r // 2)) + 1, 1 << max(r - 2, 0), top}):
                if 1 <= c <= top:
                    e = fl(code_edge(c, r))
                    mags += [np.nextafter(e, 0.0), e, np.nextafter(e, 2.0)]
            mags = [v for v in mags if 0.0 <= v < 1.0] + [0.0, np.nextafter(1.0, 0.0), 1.0]
            x = np.array(mags + [-v for v in mags])
            for scale in range(cap + 1):
                xs.append(x)
                sc.append(np.full(len(x), scale))
                sb.append(np.full(len(x), s))
                mb.append(np.full(len(x), m))
    cat = lambda v: np.concatenate(v)
    return cat(xs), cat(sc).astype(np.int64), cat(sb).astype(np.int64), cat(mb).astype(np.int64)
