"""
Content that puts every band exactly on the M/S switch's threshold (ms_stereo.py:5-27: sum|L^2 - R^2| < 0.8 sum|L^2 + R^2|),
the band tables it is cut into, the decision restated in plain additions, and the ways of getting it subtly wrong.

With R = L / 3 the two sums stand in the ratio (1 - 1/9) / (1 + 1/9) = 0.8 up to the rounding of R: the decision is made by
the last ulp of each sum, and so by the ORDER in which np.sum adds (pairwise summation: eight strided accumulators per run of
at most 128 lines combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the < 8 trailing lines one by one; longer runs split
at n // 2 rounded down to a multiple of 8) and by the two roundings of l*l - r*r.  `pairwise` writes that order out addition
by addition; the wrong variants (`sequential`, `combine_left_to_right`, `tail_first`, `split_unrounded`, `fused_terms`) are
only there so that tests/test_ms_switch_cases_cpu.py can show on the oracle alone that the content tells them apart.

Every sum here runs over the LAST axis of an array: the leading axes carry many blocks through the same additions at once
(each `+` below is one IEEE addition per block, whatever the shape).  Pure NumPy and Python; seeded; every product is
computed once and shared (callers must not write into what they get).
"""
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

from oracle import fast

import alloc_cases as ac
import settings_kit as sk

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ the sums
def _split(n, rounded=True):
    n2 = n // 2
    return n2 - n2 % 8 if rounded else n2


def _run(x, combine_in_pairs=True, tail_first=False, rounded_split=True):
    n = x.shape[-1]
    if n < 8:
        res = np.zeros(x.shape[:-1])
        for i in range(n):
            res = res + x[..., i]
        return res
    if n <= 128:
        body = n - n % 8
        r = x[..., 0:8]                                      # the eight strided accumulators, side by side
        for i in range(8, body, 8):
            r = r + x[..., i:i + 8]
        r = [r[..., j] for j in range(8)]
        if tail_first:                                       # WRONG: the trailing lines join accumulator 0 before the combine
            for i in range(body, n):
                r[0] = r[0] + x[..., i]
        if combine_in_pairs:
            res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        else:                                                # WRONG
            res = r[0]
            for j in range(1, 8):
                res = res + r[j]
        if not tail_first:
            for i in range(body, n):
                res = res + x[..., i]
        return res
    n2 = _split(n, rounded_split)                            # (not rounded: WRONG)
    return (_run(x[..., :n2], combine_in_pairs, tail_first, rounded_split) +
            _run(x[..., n2:], combine_in_pairs, tail_first, rounded_split))


def pairwise(x):
    """np.sum over a contiguous float64 run (the last axis of x), addition by addition"""
    return _run(np.asarray(x, dtype=np.float64))


def sequential(x):
    x = np.asarray(x, dtype=np.float64)
    res = np.zeros(x.shape[:-1])
    for i in range(x.shape[-1]):
        res = res + x[..., i]
    return res


def combine_left_to_right(x):
    return _run(np.asarray(x, dtype=np.float64), combine_in_pairs=False)


def tail_first(x):
    return _run(np.asarray(x, dtype=np.float64), tail_first=True)


def split_unrounded(x):
    return _run(np.asarray(x, dtype=np.float64), rounded_split=False)


def nodes(n):
    """the summation nodes (leaves + internal nodes) of a band of n lines, as mrc::ms_plan builds the tree"""
    if n <= 128:
        return 1
    n2 = _split(n)
    return nodes(n2) + nodes(n - n2) + 1


def has_unrounded_split(n):
    """a band above 128 lines whose tree holds a node with (n // 2) % 8 != 0: where split_unrounded can differ"""
    if n <= 128:
        return False
    n2 = _split(n)
    return (n // 2) % 8 != 0 or has_unrounded_split(n2) or has_unrounded_split(n - n2)


# ------------------------------------------------------------------------------------------------ the terms
def plain_terms(L, R):
    """|l*l - r*r| and |l*l + r*r|, every operation rounded (ms_stereo.py:13-16)"""
    l2, r2 = L * L, R * R
    return np.abs(l2 - r2), np.abs(l2 + r2)


def _ints(x):
    """finite float64 x -> (M, e) with x == M * 2^e, M Python integers in an object array"""
    m, e = np.frexp(x)
    return np.ldexp(m, 53).astype(np.int64).astype(object), (e - 53).astype(object)


def fused_terms(L, R):
    """WRONG: the terms as a compiler that contracts a*a +- b*b into fma(a, a, +-(b*b)) forms them, |l*l -+ fl(r*r)| rounded
    ONCE: the exact integers at the common exponent, whose conversion to float64 rounds to nearest even.  (Finite lines whose
    squares neither overflow nor underflow: no family of knife edges has others.)"""
    ml, el = _ints(L)
    mr, er = _ints(R * R)
    c = np.minimum(2 * el, er)
    ll, rr = np.left_shift(ml * ml, 2 * el - c), np.left_shift(mr, er - c)
    c = c.astype(np.int64)
    return np.abs(np.ldexp((ll - rr).astype(np.float64), c)), np.abs(np.ldexp((ll + rr).astype(np.float64), c))


def fused_difference_by_fraction(l, r):
    """the same |l*l - fl(r*r)| of two floats through fractions.Fraction (the check of fused_terms)"""
    return abs(float(Fraction(l) * Fraction(l) - Fraction(r * r)))


# ------------------------------------------------------------------------------------------------ the decision
def switch(L, R, n_lines, sum=pairwise, terms=plain_terms):
    """the switch of the blocks L, R [..., sum(n_lines)] -> int64 [..., len(n_lines)]"""
    L, R = np.asarray(L, dtype=np.float64), np.asarray(R, dtype=np.float64)
    out = np.empty(L.shape[:-1] + (len(n_lines),), np.int64)
    with np.errstate(all="ignore"):
        d, s = terms(L, R)
        lo = 0
        for i, n in enumerate(n_lines):
            out[..., i] = sum(d[..., lo:lo + n]) < 0.8 * sum(s[..., lo:lo + n])
            lo += int(n)
    return out


def _exact_sums(L, R, n_lines):
    """per band the exact integers D = sum|l^2 - r^2| and S = sum(l^2 + r^2) at a common scale -> object arrays [..., nb]"""
    L, R = np.asarray(L, dtype=np.float64), np.asarray(R, dtype=np.float64)
    D = np.empty(L.shape[:-1] + (len(n_lines),), object)
    S = np.empty_like(D)
    lo = 0
    for i, n in enumerate(n_lines):
        ml, el = _ints(L[..., lo:lo + n])
        mr, er = _ints(R[..., lo:lo + n])
        low = min(el.min(initial=0), er.min(initial=0))
        l2, r2 = np.left_shift(ml, el - low), np.left_shift(mr, er - low)
        l2, r2 = l2 * l2, r2 * r2
        D[..., i] = np.abs(l2 - r2).sum(axis=-1) if n else 0
        S[..., i] = (l2 + r2).sum(axis=-1) if n else 0
        lo += int(n)
    return D, S


def exact_margin(L, R, n_lines):
    """|d - 0.8 s| / s of every band in exact rational arithmetic (0.8 = 4/5), as float64 [..., nb]; NaN where s == 0"""
    D, S = _exact_sums(L, R, n_lines)
    out = np.full(D.shape, np.nan)
    for idx in np.ndindex(D.shape):
        if S[idx] > 0:
            out[idx] = float(Fraction(abs(5 * D[idx] - 4 * S[idx]), 5 * S[idx]))
    return out


def exact_switch(L, R, n_lines):
    """the decision in exact rational arithmetic: d < 4/5 s"""
    D, S = _exact_sums(L, R, n_lines)
    return np.array(5 * D < 4 * S, dtype=bool).astype(np.int64)


# ------------------------------------------------------------------------------------------------ band tables
BIG = (363, 390, 511, 512, 513, 693, 1000, 1024, 2048)
MAX_BANDS, MAX_NODES = 32, 64
# the library's status and words for a table beyond MAX_NODES (MRC_ERR_INVALID; mrc_ms_switch in csrc/mrc_api.cpp)
REFUSAL = (-1, "mrc_ms_switch: band table too fine (more than 64 summation nodes)")


def _pack(lengths):
    """bands into as few tables as 32 bands and 64 nodes each allow: the heaviest band first, each into the table with the
    fewest bands that still holds it (so that no table ends up with two or three bands only)"""
    count = max(-(-sum(nodes(n) for n in lengths) // MAX_NODES), -(-len(lengths) // MAX_BANDS))
    while True:
        tables = [[] for _ in range(count)]
        for n in sorted(lengths, key=lambda n: (-nodes(n), -n)):
            fits = [t for t in tables if len(t) < MAX_BANDS and sum(map(nodes, t)) + nodes(n) <= MAX_NODES]
            if not fits:
                break
            min(fits, key=len).append(n)
        else:
            return tables
        count += 1


def direct_tables():
    """name -> band lengths, for Handle.ms_switch: every length 0 .. 272 and BIG packed, a table at both limits, one band of
    one line"""
    def make():
        rng = np.random.default_rng(5)
        out = {}
        for i, t in enumerate(_pack(list(range(273)) + list(BIG))):
            out["packed%02d" % i] = tuple(int(t[j]) for j in rng.permutation(len(t)))   # long and short bands mixed
        out["full_64_nodes"] = (129, 1) * 16                  # 32 bands and 64 nodes: both limits at once
        out["one_line"] = (1,)
        for name, t in out.items():
            assert 1 <= len(t) <= MAX_BANDS and sum(map(nodes, t)) <= MAX_NODES, name
        assert sum(map(nodes, out["full_64_nodes"])) == MAX_NODES
        return out
    return _cached("direct", make)


REFUSED_TABLE = (129,) * 16 + (257,) + (1,) * 12             # 48 + 5 + 12 = 65 nodes in 29 bands
assert sum(map(nodes, REFUSED_TABLE)) == MAX_NODES + 1


def bands_of(n_lines):
    """what oracle.fast.ms_switch_batch and oracle.ms_stereo.MSSwitchSFBands read of a band table"""
    n = np.asarray(n_lines, dtype=np.int64)
    lo = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
    return SimpleNamespace(nBands=len(n), nLines=n, lowerLine=lo, upperLine=lo + n - 1)


def setting_shapes():
    """[(setting id or None, a, b)]: alloc_cases.SHAPES at the default setting, then every shape of every settings_kit
    setting"""
    return [(None, a, b) for (a, b) in ac.SHAPES] + [(sid, a, b) for sid in sk.IDS for (a, b) in sk.shapes_of(sid)]


def codec_bands(sid, a, b):
    if sid is None:
        return fast.bands_for(a, b)
    f = sk.full(sid)
    return fast.bands_for(a, b, f["n_mdct_lines"], f["sample_rate"])


def codec_shapes():
    """name -> (setting id or None, a, b): one entry per distinct band table, named after the first shape that has it"""
    def make():
        out, seen = {}, set()
        for (sid, a, b) in setting_shapes():
            t = tuple(int(v) for v in codec_bands(sid, a, b).nLines)
            if t not in seen:
                seen.add(t)
                out["%s_%dx%d" % (sid or "default", a, b)] = (sid, a, b)
        return out
    return _cached("codec_shapes", make)


def codec_tables():
    """name -> band lengths of the codec's own tables"""
    return _cached("codec", lambda: {k: tuple(int(v) for v in codec_bands(*v3).nLines) for k, v3 in codec_shapes().items()})


def all_tables():
    return dict(direct_tables(), **codec_tables())


# ------------------------------------------------------------------------------------------------ content
EDGE_FAMILIES = ("third", "triple", "signed", "mixed")      # every band a knife edge, scales 2^-6 .. 1
FAMILIES = EDGE_FAMILIES + ("wide", "beside", "special")
SPECIAL = ("zeros", "minus_zeros", "denormal_lines", "squares_underflow", "squares_denormal", "squares_overflow", "nan",
           "inf")


def n_blocks(n_lines, family="third"):
    """blocks per table: 32, more where a table has few bands (about 1000 decisions per family at least); four times as many
    of `triple`, where fused terms flip 4 to 5 % of the decisions only (l*l is the small square there, and its second
    rounding seldom shows), so that the share of a table stays clear of the 3 % asked of it"""
    return max(32, -(-1024 // len(n_lines))) * (4 if family == "triple" else 1)


def _base(rng, n, total, lowest):
    x = rng.normal(0.0, 0.1, (n, total)) * np.ldexp(1.0, rng.integers(lowest, 1, (n, total)))
    return np.clip(x, -0.89, 0.89)                             # (never reached: |R|, |L| < 0.9 whatever the draw)


def _special(total, n_lines):
    band = np.repeat(np.arange(len(n_lines)), n_lines)
    mid = band == int(np.argmax(n_lines))                      # one band: the longest
    sign = np.where(np.arange(total) % 2 == 0, 1.0, -1.0)
    L = np.zeros((len(SPECIAL), total))
    L[1] = -0.0
    for row, v in ((2, 1e-310), (3, 1e-170), (4, 1e-160), (5, 1e160)):
        L[row] = v * sign * (1.0 + np.arange(total) % 7)
    R = L / 3.0
    R[1] = -0.0
    for row, v in ((6, np.nan), (7, np.inf)):
        L[row] = 0.05 * sign
        R[row] = L[row] / 3.0
        L[row, mid] = v
    return L, R


def content(n_lines, family):
    """L, R [n_blocks][sum(n_lines)] float64 of the family on the table (read-only)"""
    n_lines = tuple(int(v) for v in n_lines)

    def make():
        total, n = sum(n_lines), n_blocks(n_lines, family)
        rng = np.random.default_rng([2025, FAMILIES.index(family), len(n_lines), total, n_lines[0], n_lines[-1]])
        if family == "special":
            L, R = _special(total, n_lines)
        else:
            x = _base(rng, n, total, -40 if family == "wide" else -6)
            third = x / 3.0
            if family in ("third", "wide"):
                L, R = x, third
            elif family == "triple":
                L, R = third, x
            elif family == "signed":
                L, R = x, third * rng.choice([-1.0, 1.0], (n, total))
            elif family == "mixed":
                swap = rng.random((n, total)) < 0.5
                L, R = np.where(swap, third, x), np.where(swap, x, third)
            elif family == "beside":
                off = 1.0 + 1e-9 * rng.choice([-1.0, 1.0], (n, len(n_lines)))
                L, R = x, third * np.repeat(off, n_lines, axis=1)
            else:
                raise ValueError(family)
        L.setflags(write=False)
        R.setflags(write=False)
        return L, R
    return _cached(("content", n_lines, family), make)


def oracle_switch(n_lines, family):
    """oracle.fast.ms_switch_batch on the family's blocks of the table -> int64 [n_blocks][nb] (read-only)"""
    n_lines = tuple(int(v) for v in n_lines)

    def make():
        L, R = content(n_lines, family)
        with np.errstate(all="ignore"):
            sw = fast.ms_switch_batch(L, R, bands_of(n_lines))
        sw.setflags(write=False)
        return sw
    return _cached(("oracle", n_lines, family), make)


# ------------------------------------------------------------------------------------------------ back-end blocks
BACKEND_BLOCKS = 16
BACKEND_FAMILIES = EDGE_FAMILIES + ("wide", "beside")


def backend_configs():
    """the joint configurations of alloc_cases.CONFIGS, then (a, b, True, tbps, setting id) for the joint shapes of every
    settings_kit setting: alloc_cases.layout takes both"""
    out = [cfg for cfg in ac.CONFIGS if cfg[2]]
    for sid in sk.IDS:
        out += [(a, b, True, sk.full(sid)["target_bits_per_sample"], sid) for (a, b) in sk.shapes_of(sid)]
    return out


def backend_cases(cfg):
    """16 joint blocks on the threshold for mrc_dev_alloc_quant and its chained form, assembled as alloc_cases.cases are
    (the oracle's switch selects SMRs and coded lines), and the oracle's integers for them"""
    def make():
        lay = ac.layout(cfg)
        n_lines, nb, half = tuple(int(v) for v in lay["sfb"].nLines), lay["nb"], lay["half"]
        n = BACKEND_BLOCKS
        lines = np.empty((n, 4, half))
        for i in range(n):
            L, R = content(n_lines, BACKEND_FAMILIES[i % len(BACKEND_FAMILIES)])
            lines[i, 0], lines[i, 1] = L[i], R[i]
        lines[:, 2] = (lines[:, 0] + lines[:, 1]) / 2.0
        lines[:, 3] = (lines[:, 0] - lines[:, 1]) / 2.0
        rng = np.random.default_rng([2026, cfg[0], cfg[1], int(round(100 * cfg[3]))])
        vectors = np.stack([ac.family_smr("normal", lay["n_tot"], nb, rng) for _ in range(n)])
        c = ac._assemble(cfg, np.full(n, ac.FAMILIES.index("normal")), vectors, lines, np.zeros((n, 4), np.int64))
        c["reservoir"] = np.where((np.arange(n) // 2) % 2 == 0, 0, 1000).astype(np.int64)
        bits = np.empty((n, lay["n_tot"]), np.int64)
        left = np.empty(n, np.int64)
        for i in range(n):
            bi, li = ac.BitAlloc(ac.budget_of(cfg, c["reservoir"][i]), lay["max_mant"], lay["n_tot"], lay["n_lines"],
                                 vectors[i].copy())
            bits[i], left[i] = bi.astype(np.int64), li
        sf, mant = ac._quantise(cfg, c["coded"], bits)
        want = dict(ms_switch=c["ms_switch"], bit_alloc=bits.reshape(n, 2, nb), reservoir_out=left, scale_factor=sf,
                    mantissa=mant)
        return c, want
    return _cached(("backend",) + tuple(cfg), make)
