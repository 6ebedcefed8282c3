"""
Crafted blocks for the constant-quality VBR kernels (vbr_alloc_kernel, vbr_profile_kernel, vbr_pick_kernel; the rule:
DESIGN.md section 12, restated in tests/vbr_restatement.py): what numbers computed from audio never are.  Pure NumPy and the
oracle; seeded; every product is computed once per configuration and shared (callers must not write into what they get).

A configuration is (a, b, joint, setting): a block shape, the channel mode and a handle -- "default" (maxMantBits 16), "F"
(scale factor field of one bit, maxMantBits 8), "H" (maxMantBits 2: candidates {0, 2}), "192k" (a band table with bands
without lines).  Its blocks cross, by seeded draws:

  lines     per signal plane band peaks random | 2^-k | one ulp under | one ulp over (tests/alloc_cases.py's lines), bands of
            zeros, whole blocks of zeros, overall scales from {0, 3, 15} (cut to the field's width); joint blocks: the S plane
            independent | bit-equal to M with the same overall scale | 0 | M = 0 | S = 2^-12 M
  X         per band and output channel: the planes themselves | the planes plus a perturbation of 2^-9 of the band's peak
            (the noise never vanishes) | the decoded lines of one state n* of the walk (the noise is exactly 0 there)
  T (dB)    per output channel: flat | uniform in [-30, 90] | +inf from a line inside a band upwards and on one line below |
            200 (every band fits at 0 bits) | -30
  switch    all 0 | all 1 | alternating | random
  ceiling   +inf | 0 (twice as often) | four finite values 20 dB apart, drawn per configuration
"""
import math

import numpy as np

import alloc_cases as ac
import vbr_restatement as vr
from oracle import codec

SETTINGS = {"default": {}, "F": dict(n_scale_bits=1, n_mant_size_bits=3), "H": dict(n_mant_size_bits=1),
            "192k": dict(sample_rate=192000)}
CONFIGS = ([(a, b, j, "default") for (a, b) in ac.SHAPES for j in (False, True)] +
           [(a, a, j, s) for s in ("F", "H") for a in (1024, 128) for j in (False, True)] +
           [(128, 128, j, "192k") for j in (False, True)])
N_BLOCKS = 168
N_FINITE = 4
NEED = 20                                                    # cases of every branch a configuration can hold
JOINT_KINDS = ("independent", "s_equals_m", "s_zero", "m_zero", "s_small")
X_KINDS = ("exact", "perturbed", "decoded")
T_KINDS = ("flat", "uniform", "inf_top", "high", "low")
BRANCHES = ("stop_at_0", "stop_interior", "stop_at_max_fitting", "capped", "lr_streams_differ", "lr_one_stream_capped",
            "ms_exact_tie_raised", "ms_e1_larger", "ms_pick_switched", "ms_capped", "ms_past_step_16", "band_of_zeros",
            "mask_inf", "band_without_lines", "block_c_inf", "block_c_zero_noise")
_CACHE = {}


def config_id(cfg):
    a, b, joint, s = cfg
    return "%dx%d-%s-%s" % (a, b, "joint" if joint else "mono", s)


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def layout(cfg):
    a, b, joint, s = cfg

    def make():
        kw = SETTINGS[s]
        rate = kw.get("sample_rate", 48000)
        nsb, nmsb = kw.get("n_scale_bits", 4), kw.get("n_mant_size_bits", 4)
        sfb = codec.bands_for_block(a, b, 1024, rate)
        n_lines = np.asarray(sfb.nLines, np.int64)
        return dict(sfb=sfb, nb=sfb.nBands, half=(a + b) // 2, ns=2 if joint else 1, nsig=4 if joint else 1, nsb=nsb,
                    max_bits=min(16, 1 << nmsb), n_lines=n_lines, edges=np.concatenate([[0], np.cumsum(n_lines)]),
                    band_of=np.repeat(np.arange(sfb.nBands), n_lines), handle=dict(kw))
    return _cached(("layout",) + tuple(cfg), make)


def impossible(cfg):
    """the branches a configuration cannot hold"""
    lay = layout(cfg)
    out = set()
    if not cfg[2]:                                            # mono has no L/R pair and no M/S band
        out |= {b for b in BRANCHES if b.startswith(("lr_", "ms_"))}
    if lay["max_bits"] != 16:                                 # fewer than 17 steps
        out.add("ms_past_step_16")
    if lay["max_bits"] == 2 and not cfg[2]:                   # candidates {0, 2}: nothing between them (an M/S band: (2, 0))
        out.add("stop_interior")
    if (lay["n_lines"] > 0).all():                            # only 192 kHz has empty bands
        out.add("band_without_lines")
    return out


def _seed(cfg, what):
    return [what, cfg[0], cfg[1], int(cfg[2]), sorted(SETTINGS).index(cfg[3])]


def ceilings(cfg):
    """the configuration's ceilings: +inf, 0 and N_FINITE values 20 dB apart from 1e-3 (each moved by up to 3 dB)"""
    rng = np.random.default_rng(_seed(cfg, 5))
    return np.concatenate([[math.inf, 0.0], 10.0 ** (-3.0 + 2.0 * np.arange(N_FINITE) + rng.uniform(-0.3, 0.3, N_FINITE))])


def _plane(lay, kind, osc, rng, edge):
    """one signal plane, unscaled: |line * 2^osc| < 1"""
    nb, half = lay["nb"], lay["half"]
    k = rng.integers(1, 24, nb)
    p2 = np.ldexp(1.0, -k)
    peak = [rng.uniform(1e-6, 0.999, nb), p2, np.nextafter(p2, 0.0), np.nextafter(p2, 1.0)][kind]
    peak = np.where(rng.random(nb) < 0.15, 0.0, peak)         # some bands all zero
    x = edge[rng.integers(0, len(edge), half)] * peak[lay["band_of"]]
    full = lay["n_lines"] > 0
    at = (lay["edges"][:-1] + rng.integers(0, np.maximum(lay["n_lines"], 1)))[full]
    x[at] = (peak * rng.choice([-1.0, 1.0], nb))[full]
    return np.ldexp(x, -int(osc))


def _walk_states(lay, pair):
    """the states (n0, n1) an M/S band passes, from the two streams' bands alone (the picks need neither X nor T)"""
    n, out = [0, 0], [(0, 0)]
    mb = lay["max_bits"]
    while True:
        e = [pair[s].error(n[s]) for s in range(2)]
        pick = 1 if e[1] > e[0] else 0
        if n[pick] >= mb:
            pick ^= 1
        if n[pick] >= mb:
            return out
        n[pick] = n[pick] + 1 if n[pick] else 2
        out.append(tuple(n))


def _make_block(cfg, i, rng, edge):
    lay = layout(cfg)
    nb, half, ns, nsig, nsb, mb, joint = lay["nb"], lay["half"], lay["ns"], lay["nsig"], lay["nsb"], lay["max_bits"], cfg[2]
    e = lay["edges"]
    cap = (1 << nsb) - 1
    osc = np.minimum(rng.choice([0, 3, 15], size=nsig), cap)
    line_kind = int(rng.integers(0, 4))
    jk = JOINT_KINDS[int(rng.integers(0, len(JOINT_KINDS)))] if joint else None
    lines = np.stack([_plane(lay, line_kind, osc[s], rng, edge) for s in range(nsig)])
    if rng.random() < 0.04:
        lines[:] = 0.0                                        # a whole block of zeros
    if jk == "s_equals_m":
        osc[3] = osc[2]
        lines[3] = lines[2]
    elif jk == "s_zero":
        lines[3] = 0.0
    elif jk == "m_zero":
        lines[2] = 0.0
    elif jk == "s_small":
        osc[3] = osc[2]
        lines[3] = np.ldexp(lines[2], -12)
    ms = None
    if joint:
        pattern = int(rng.integers(0, 4))
        ms = [np.zeros(nb, int), np.ones(nb, int), np.arange(nb) % 2, rng.integers(0, 2, nb)][pattern].astype(np.int64)
    # ---- X: per band and channel
    cand = vr.candidates(mb)
    X = np.zeros((ns, half))
    xk = rng.integers(0, len(X_KINDS), (ns, nb))
    for j in range(nb):
        lo, hi = e[j], e[j + 1]
        if hi == lo:
            continue
        is_ms = joint and ms[j] == 1
        if is_ms:
            base = [lines[2, lo:hi] + lines[3, lo:hi], lines[2, lo:hi] - lines[3, lo:hi]]
            xk[1, j] = xk[0, j]                               # (one state of the pair decides both channels)
        else:
            base = [lines[s, lo:hi] for s in range(ns)]
        dec = None
        if X_KINDS[xk[0, j]] == "decoded" or (not is_ms and ns == 2 and X_KINDS[xk[1, j]] == "decoded"):
            last = rng.random() < 0.35                        # n*: the last state rather often (it must fit there, uncapped)
            if is_ms:
                pair = [vr._Band(np.ldexp(lines[2 + s, lo:hi], int(osc[2 + s])), 1 << int(osc[2 + s]), nsb) for s in range(2)]
                states = _walk_states(lay, pair)
                n0, n1 = states[-1 if last else int(rng.integers(0, len(states)))]
                d0, d1 = pair[0].decoded(n0), pair[1].decoded(n1)
                dec = [d0 + d1, d0 - d1]
            else:
                dec = []
                for s in range(ns):
                    n = cand[-1 if last else int(rng.integers(0, len(cand)))]
                    dec.append(vr._Band(np.ldexp(lines[s, lo:hi], int(osc[s])), 1 << int(osc[s]), nsb).decoded(n))
        for ch in range(ns):
            kind = X_KINDS[xk[ch, j]]
            if kind == "exact":
                X[ch, lo:hi] = base[ch]
            elif kind == "perturbed":
                amp = max(np.max(np.abs(base[ch])), 2.0 ** -30) * 2.0 ** -9
                X[ch, lo:hi] = base[ch] + amp * rng.choice([-1.0, 1.0], hi - lo) * rng.uniform(0.5, 1.0, hi - lo)
            else:
                X[ch, lo:hi] = dec[ch]
    # ---- T: per channel
    T = np.zeros((ns, half))
    tk = rng.integers(0, len(T_KINDS), ns)
    for ch in range(ns):
        kind = T_KINDS[tk[ch]]
        if kind == "flat":
            T[ch] = rng.uniform(-10.0, 70.0)
        elif kind == "uniform":
            T[ch] = rng.uniform(-30.0, 90.0, half)
        elif kind == "inf_top":
            T[ch] = rng.uniform(-30.0, 90.0, half)
            cut = int(rng.integers(half // 4, half))
            T[ch, cut:] = math.inf                            # the band of `cut` partly, the bands above wholly infinite
            T[ch, int(rng.integers(0, cut))] = math.inf       # and a single line of a band below
        elif kind == "high":
            T[ch] = 200.0
        else:
            T[ch] = -30.0
    return dict(lines=lines, osc=osc.astype(np.int64), ms=ms, X=X, T=T, joint_kind=jk, x_kind=xk, t_kind=tk)


MAX_DRAWS = 12


def _restate_block(cfg, blk, c, profile=False):
    lay = layout(cfg)
    return vr.block_crafted(blk["lines"], blk["osc"], blk["ms"], blk["X"], blk["T"], c, lay["sfb"], lay["nsb"], lay["max_bits"],
                            profile=profile)


def _build(cfg):
    """Block after block: draw it, restate it at its ceiling (and without one), and draw it again if a decision of either
    walk is an edge candidate -- a ratio within 1e-6 of the ceiling, two unequal error energies within 1e-6 of each other
    (planes with peaks an ulp from 2^-k make those by themselves)."""
    def make():
        rng = np.random.default_rng(_seed(cfg, 4))
        edge = ac._edge_values()
        cl = ceilings(cfg)
        which = rng.permutation(np.append(np.arange(len(cl)), 1)[np.arange(N_BLOCKS) % (len(cl) + 1)])   # c = 0 twice as often
        blocks, refs, redrawn = [], [], 0
        for i in range(N_BLOCKS):
            for draw in range(MAX_DRAWS):
                blk = _make_block(cfg, i, rng, edge)
                ref = _restate_block(cfg, blk, cl[which[i]], profile=True)
                if ref["edges"] == 0:
                    break
                redrawn += 1
            blocks.append(blk); refs.append(ref)
        cs = dict(lines=np.stack([b["lines"] for b in blocks]), overall_scale=np.stack([b["osc"] for b in blocks]),
                  ms_switch=np.stack([b["ms"] for b in blocks]) if cfg[2] else None,
                  X=np.stack([b["X"] for b in blocks], axis=1), T=np.stack([b["T"] for b in blocks], axis=1), ceiling=which,
                  joint_kind=[b["joint_kind"] for b in blocks], x_kind=np.stack([b["x_kind"] for b in blocks]),
                  t_kind=np.stack([b["t_kind"] for b in blocks]))
        for v in cs.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        rf = dict(blocks=refs, ceilings=cl, redrawn=redrawn, edges=sum(b["edges"] for b in refs),
                  bit_alloc=np.stack([b["bit_alloc"] for b in refs]), scale_factor=np.stack([b["scale_factor"] for b in refs]),
                  mantissa=np.stack([b["mantissa"] for b in refs]), capped=np.array([b["capped"] for b in refs]))
        return cs, rf
    return _cached(("build",) + tuple(cfg), make)


def cases(cfg):
    """N_BLOCKS blocks: lines [n][nsig][half], overall_scale [n][nsig], ms_switch [n][nb] (None: mono), X / T [ns][n][half]
    (as the kernels read them: left rows, then right rows), ceiling [n] (index into ceilings(cfg)), the families drawn"""
    return _build(cfg)[0]


def reference(cfg):
    """the restatement on every block at its own ceiling, with the walk without a ceiling under "profile": dict(blocks (list
    of block_crafted's dicts), ceilings, redrawn (blocks drawn again), edges (0), bit_alloc [n][ns][nb], scale_factor,
    mantissa [n][ns][half], capped [n])"""
    return _build(cfg)[1]


def restate(cfg, i, c, profile=False):
    """the restatement on block i of the configuration at another linear ceiling c"""
    cs = cases(cfg)
    blk = dict(lines=cs["lines"][i], osc=cs["overall_scale"][i], ms=cs["ms_switch"][i] if cfg[2] else None, X=cs["X"][:, i],
               T=cs["T"][:, i])
    return _restate_block(cfg, blk, c, profile)


def record(cfg, width):
    """the walks without a ceiling as vbr_profile_kernel records them: ratios [n][nb][width] (NaN where nothing is written),
    picks [n][nb] -- width: Handle.vbr_record_width(joint)"""
    def make():
        lay, ref, cs = layout(cfg), reference(cfg), cases(cfg)
        nb, joint = lay["nb"], cfg[2]
        state = lambda n: n - 1 if n else 0
        rat = np.full((N_BLOCKS, nb, width), np.nan)
        picks = np.zeros((N_BLOCKS, nb), np.int64)
        for i, blk in enumerate(ref["blocks"]):
            p = blk["profile"]
            for j in range(nb):
                if joint and cs["ms_switch"][i][j] == 1:
                    for step, (_, r0, r1) in enumerate(p["trail"][0][j]):
                        rat[i, j, 2 * step], rat[i, j, 2 * step + 1] = r0, r1
                    picks[i, j] = sum(s << k for k, s in enumerate(p["raised"][j]))
                else:
                    for s in range(lay["ns"]):
                        for (n, r) in p["trail"][s][j]:
                            rat[i, j, s * (width // 2 if joint else 0) + state(n)] = r
        return rat, picks
    return _cached(("record", width) + tuple(cfg), make)


def branch_counts(cfg):
    """how often the blocks of the configuration, at their own ceilings, take every branch of BRANCHES"""
    lay, cs, ref = layout(cfg), cases(cfg), reference(cfg)
    nb, ns, mb, joint = lay["nb"], lay["ns"], lay["max_bits"], cfg[2]
    hit = dict.fromkeys(BRANCHES, 0)
    for i, blk in enumerate(ref["blocks"]):
        c = ref["ceilings"][cs["ceiling"][i]]
        ba, caps = blk["bit_alloc"], blk["caps"]
        zero_noise = False
        for j in range(nb):
            lo, hi = lay["edges"][j], lay["edges"][j + 1]
            if hi == lo:
                hit["band_without_lines"] += 1
                continue
            is_ms = joint and cs["ms_switch"][i][j] == 1
            sigs = [2, 3] if is_ms else list(range(ns))
            hit["band_of_zeros"] += all(not cs["lines"][i][s, lo:hi].any() for s in sigs)
            hit["mask_inf"] += sum(math.isinf(blk["masks"][ch][j]) for ch in range(ns))
            if is_ms:
                cap = caps[0, j]
                hit["ms_capped"] += cap
                hit["capped"] += cap
                if not cap:
                    n = tuple(ba[:, j])
                    hit["stop_at_0"] += n == (0, 0)
                    hit["stop_at_max_fitting"] += n == (mb, mb)
                    hit["stop_interior"] += n not in ((0, 0), (mb, mb))
                    zero_noise |= n != (0, 0) and blk["ratio"][0, j] == 0.0 and blk["ratio"][1, j] == 0.0 and \
                        not math.isinf(blk["masks"][0][j]) and not math.isinf(blk["masks"][1][j])
                steps = blk["steps"][j]
                hit["ms_exact_tie_raised"] += any(e0 == e1 and e0 > 0 and took is not None for (e0, e1, _, took) in steps)
                hit["ms_e1_larger"] += any(e1 > e0 for (e0, e1, _, _) in steps)
                hit["ms_pick_switched"] += any(took is not None and took != larger for (_, _, larger, took) in steps)
                hit["ms_past_step_16"] += len(blk["trail"][0][j]) > 17
                continue
            for s in range(ns):
                hit["capped"] += caps[s, j]
                if not caps[s, j]:
                    hit["stop_at_0"] += ba[s, j] == 0
                    hit["stop_at_max_fitting"] += ba[s, j] == mb
                    hit["stop_interior"] += 0 < ba[s, j] < mb
                    zero_noise |= ba[s, j] > 0 and blk["ratio"][s, j] == 0.0 and not math.isinf(blk["masks"][s][j])
            if joint:
                hit["lr_streams_differ"] += ba[0, j] != ba[1, j]
                hit["lr_one_stream_capped"] += caps[0, j] + caps[1, j] == 1
        hit["block_c_inf"] += math.isinf(c) and not ba.any()
        hit["block_c_zero_noise"] += c == 0.0 and bool(zero_noise)
    return hit
