"""
Crafted inputs of the bit-allocation back ends (bitalloc.py:106-155 restated three times on the device): SMRs that tie, tie
again after every grant or sit an ulp from a 6 dB boundary, budgets around zero, around the smallest band and beyond what
fills every band, and lines whose band peaks sit on and beside powers of two.  Pure NumPy and the oracle; seeded; every
product is computed once per configuration and shared (callers must not write into what they get).

A configuration is (a, b, joint, tbps): a block shape, the channel mode and the handle's target bits per sample (2.86: the
default, fractional budgets; 3.0: integer budgets, where nLines == bitsLeft and bitsLeft == 0 can happen).  Its cases are
every SMR family crossed with every reservoir, in a seeded random order (so that the first 1, 63, 64, 65 cases are mixed).
"""
import numpy as np

from oracle import fast
from oracle.bitalloc import BitAlloc, _DEAD

SHAPES = [(1024, 1024), (128, 128), (1024, 128), (128, 1024)]
TBPS = [2.86, 3.0]
CONFIGS = [(a, b, joint, t) for (a, b) in SHAPES for joint in (False, True) for t in TBPS]
MAX_MANT = 16                                                # min(16, 1 << nMantSizeBits) at the default 4
N_SCALE_BITS = 4
FAMILIES = ("zero", "minus_zero", "equal_7.3", "six_k", "six_k_ulp", "normal", "dominant", "ramp_up", "ramp_down",
            "tie_group_edge", "tie_first_last", "tie_across_streams", "large")
_CACHE = {}


def config_id(cfg):
    a, b, joint, t = cfg
    return "%dx%d-%s-%s" % (a, b, "joint" if joint else "mono", t)


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def params(tbps):
    return dict(fast.DEFAULTS, targetBitsPerSample=tbps)


def group_size(n_tot):
    """alloc_group_size of csrc/mrc_kernels_alloc.hip: the bands per group of the two-level argmax"""
    return 4 if n_tot <= 16 else 6 if n_tot <= 32 else 8


def layout(cfg):
    """the band table and sizes of a configuration (with a fifth entry, a setting of tests/settings_kit.py: that setting's)"""
    a, b, joint, tbps = cfg[:4]

    def make():
        P, max_mant = params(tbps), MAX_MANT
        if len(cfg) > 4:
            import settings_kit as sk
            f = sk.full(cfg[4])
            P = dict(sampleRate=f["sample_rate"], nMDCTLines=f["n_mdct_lines"], nScaleBits=f["n_scale_bits"],
                     nMantSizeBits=f["n_mant_size_bits"], targetBitsPerSample=tbps, blkswBitA=f["blksw_bits_a"],
                     blkswBitB=f["blksw_bits_b"])
            max_mant = sk.max_mant_bits(cfg[4])
        sfb = fast.bands_for(a, b, P["nMDCTLines"], P["sampleRate"])
        nb, half = sfb.nBands, (a + b) // 2
        ns = 2 if joint else 1
        n_lines = np.tile(np.asarray(sfb.nLines, dtype=np.int64), ns)
        base = fast.joint_budget(P, half, nb, 0) if joint else fast.mono_budget(P, half, nb)
        return dict(sfb=sfb, nb=nb, half=half, ns=ns, nsig=4 if joint else 1, n_tot=ns * nb, n_lines=n_lines, base=base,
                    fill=max_mant * int(n_lines.sum()), P=P, max_mant=max_mant, n_scale_bits=P["nScaleBits"])
    return _cached(("layout",) + tuple(cfg), make)


def budget_of(cfg, reservoir):
    """codecThem.py:299-308 / 381-396: the budget of a block that starts with `reservoir`"""
    lay = layout(cfg)
    if cfg[2]:
        return fast.joint_budget(lay["P"], lay["half"], lay["nb"], int(reservoir))
    return fast.mono_budget(lay["P"], lay["half"], lay["nb"]) + int(reservoir)


# ------------------------------------------------------------------------------------------------ SMR families
def family_smr(name, n_tot, nb, rng):
    """one SMR vector [n_tot] of the family (stream 0's bands, then stream 1's)"""
    if name == "zero":
        return np.zeros(n_tot)
    if name == "minus_zero":
        return np.full(n_tot, -0.0)
    if name == "equal_7.3":
        return np.full(n_tot, 7.3)
    if name in ("six_k", "six_k_ulp"):
        s = 6.0 * rng.integers(-5, 13, n_tot)
        if name == "six_k_ulp":
            how = rng.integers(0, 5, n_tot)
            s = np.choose(how, [s, np.nextafter(s, -np.inf), s + 1e-13, s - 1e-13, s + 2.0 ** -40])
        return s
    if name == "normal":
        return rng.normal(10.0, 15.0, n_tot)
    if name == "dominant":
        s = np.full(n_tot, -100.0)
        s[rng.integers(0, n_tot)] = 200.0
        return s
    if name in ("ramp_up", "ramp_down"):
        s = rng.integers(-2, 6) * 6.0 + (6.0 / n_tot) * np.arange(n_tot)
        return s if name == "ramp_up" else s[::-1].copy()
    if name.startswith("tie_"):
        s = rng.normal(10.0, 15.0, n_tot)
        top = np.ceil(s.max()) + 3.0
        if name == "tie_group_edge":
            gs = group_size(n_tot)
            g = int(rng.integers(1, (n_tot + gs - 1) // gs))
            where = (g * gs - 1, g * gs)
        elif name == "tie_first_last":
            where = (0, n_tot - 1)
        else:
            where = (nb - 1, nb % n_tot)                         # (mono: the last band and band 0)
        s[list(where)] = top
        return s
    if name == "large":
        return 1e5 * rng.integers(-1, 2, n_tot) + 6.0 * rng.integers(0, 3, n_tot)
    raise ValueError(name)


def reservoirs(cfg, rng):
    lay = layout(cfg)
    b0, fill = int(lay["base"]), lay["fill"]
    r = [-10 ** 6, -b0 - 3, -b0 - 1, -b0, -b0 + 1]
    r += [-b0 + j for j in range(25)]
    r += [int(v) for v in rng.integers(-b0 - 50, fill - b0 + 51, 40)]
    r += [fill, 10 ** 6]
    return np.asarray(r, dtype=np.int64)


# ------------------------------------------------------------------------------------------------ lines
def _edge_values():
    def make():
        import os
        v = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quantize.npz"))["vals"]
        return v[np.abs(v) <= 1.0]
    return _cached("edge_values", make)


def make_lines(cfg, n, rng):
    """-> lines [n][nsig][half] (unscaled), overall_scale [n][nsig].  |line * 2^overall_scale| < 1 for every signal.  Joint:
    per band R = L (switch on) or R = 0 (off), M and S independent data.  (On these two inputs every order of summation
    gives the same switch: the decisions themselves are exercised by tests/ms_switch_cases.py, whose bands sit on the
    threshold.)"""
    lay = layout(cfg)
    sfb, nb, half, nsig, joint = lay["sfb"], lay["nb"], lay["half"], lay["nsig"], cfg[2]
    edge = _edge_values()
    osc = rng.choice([0, 3, (1 << N_SCALE_BITS) - 1], size=(n, nsig))
    down = osc.max(axis=1) if joint else osc[:, 0]            # L and R share lines: both scales must keep them below 1
    lines = np.zeros((n, nsig, half))
    band_of = np.repeat(np.arange(nb), sfb.nLines)
    for i in range(n):
        kind = i % 4                                          # the band peaks: random | 2^-k | one ulp under | one ulp over
        for sig in ([0, 2, 3] if joint else [0]):
            k = rng.integers(1, 24, nb)
            p2 = np.ldexp(1.0, -k)
            peak = [rng.uniform(1e-6, 0.999, nb), p2, np.nextafter(p2, 0.0), np.nextafter(p2, 1.0)][kind]
            peak = np.where(rng.random(nb) < 0.15, 0.0, peak)  # some bands all zero
            x = edge[rng.integers(0, len(edge), half)] * peak[band_of]
            at = np.asarray(sfb.lowerLine) + rng.integers(0, np.asarray(sfb.nLines))
            x[at] = peak * rng.choice([-1.0, 1.0], nb)
            lines[i, sig] = np.ldexp(x, -int(down[i] if sig == 0 else osc[i, sig]))
        if joint:
            pattern = (i // 4) % 4                            # the switch: all on | all off | alternating | random
            on = [np.ones(nb, bool), np.zeros(nb, bool), np.arange(nb) % 2 == 0, rng.random(nb) < 0.5][pattern]
            lines[i, 1] = np.where(on[band_of], lines[i, 0], 0.0)
    return lines, osc.astype(np.int64)


# ------------------------------------------------------------------------------------------------ cases of a configuration
def _assemble(cfg, fam_idx, vectors, lines, osc):
    """SMR vectors [n][n_tot] -> the device's smr [n][nsig][nb] (unselected signals NaN), the oracle's switch and the
    selected scaled lines"""
    lay = layout(cfg)
    sfb, nb, nsig, joint = lay["sfb"], lay["nb"], lay["nsig"], cfg[2]
    n = len(vectors)
    scaled = lines * np.ldexp(1.0, osc)[:, :, None]
    assert (np.abs(scaled) < 1.0).all()
    if joint:
        sw = fast.ms_switch_batch(lines[:, 0], lines[:, 1], sfb)
        on = sw == 1
        smr = np.full((n, 4, nb), np.nan)
        v0, v1 = vectors[:, :nb], vectors[:, nb:]
        smr[:, 0][~on] = v0[~on]; smr[:, 2][on] = v0[on]
        smr[:, 1][~on] = v1[~on]; smr[:, 3][on] = v1[on]
        on_line = on[:, np.repeat(np.arange(nb), sfb.nLines)]
        coded = np.stack([np.where(on_line, scaled[:, 2], scaled[:, 0]), np.where(on_line, scaled[:, 3], scaled[:, 1])], axis=1)
    else:
        sw = None
        smr = vectors[:, None, :].copy()
        coded = scaled
    return dict(family=fam_idx, vectors=vectors, smr=smr, lines=lines, overall_scale=osc, ms_switch=sw, coded=coded)


def cases(cfg):
    """every family x every reservoir, shuffled: dict of vectors [n][n_tot], smr [n][nsig][nb], reservoir [n], budget [n],
    lines [n][nsig][half], overall_scale [n][nsig], ms_switch [n][nb] or None, coded [n][ns][half] (selected scaled lines)"""
    def make():
        lay = layout(cfg)
        rng = np.random.default_rng([2024, cfg[0], cfg[1], int(cfg[2]), int(round(100 * cfg[3]))])
        res = reservoirs(cfg, rng)
        fam = np.repeat(np.arange(len(FAMILIES)), len(res))
        r = np.tile(res, len(FAMILIES))
        order = rng.permutation(len(fam))
        fam, r = fam[order], r[order]
        vectors = np.stack([family_smr(FAMILIES[f], lay["n_tot"], lay["nb"], rng) for f in fam])
        assert np.isfinite(vectors).all() and np.abs(vectors).max() <= 1.1e5
        lines, osc = make_lines(cfg, len(fam), rng)
        out = _assemble(cfg, fam, vectors, lines, osc)
        out["reservoir"] = r
        out["budget"] = np.array([budget_of(cfg, v) for v in r])
        return out
    return _cached(("cases",) + tuple(cfg), make)


def _quantise(cfg, coded, bits):
    """fast._quantise_batch per stream -> scale_factor [n][ns][nb], mantissa [n][ns][half]"""
    lay = layout(cfg)
    nb = lay["nb"]
    sf, mant = zip(*[fast._quantise_batch(coded[:, s], bits[:, s * nb:(s + 1) * nb], lay["sfb"], lay["n_scale_bits"])
                     for s in range(lay["ns"])])
    return np.stack(sf, axis=1), np.stack(mant, axis=1)


def reference(cfg):
    """the oracle on every case: bit_alloc [n][ns][nb], reservoir_out [n], smr_after [n][n_tot] (the running SMRs the loop
    leaves in place), scale_factor, mantissa"""
    def make():
        lay, c = layout(cfg), cases(cfg)
        n = len(c["reservoir"])
        bits = np.empty((n, lay["n_tot"]), np.int64)
        left = np.empty(n, np.int64)
        after = c["vectors"].copy()
        for i in range(n):
            bi, li = BitAlloc(c["budget"][i], MAX_MANT, lay["n_tot"], lay["n_lines"], after[i])
            bits[i], left[i] = bi.astype(np.int64), li
        sf, mant = _quantise(cfg, c["coded"], bits)
        return dict(bit_alloc=bits.reshape(n, lay["ns"], lay["nb"]), reservoir_out=left, smr_after=after, scale_factor=sf,
                    mantissa=mant)
    return _cached(("reference",) + tuple(cfg), make)


# ------------------------------------------------------------------------------------------------ the instrumented loop
EVENTS = ("tie", "two_bit_negative", "retired_no_bits", "retired_full", "no_iteration", "all_retired", "negative_out",
          "lines_equal_left", "left_zero_after_grant")


def instrumented(budget, max_mant, n_bands, n_lines, smr):
    """oracle.bitalloc.BitAlloc with every branch counted -> (bits, int(left), counts by EVENTS)"""
    running = smr.copy()
    left = budget
    retired = 0
    bits = np.zeros(n_bands)
    hit = dict.fromkeys(EVENTS, 0)
    if not left > 0:
        hit["no_iteration"] = 1
    while left > 0:
        i = np.argmax(running)
        top = running[i]
        if top != _DEAD and np.count_nonzero(running == top) > 1:
            hit["tie"] += 1
        if bits[i] < max_mant and n_lines[i] <= left:
            if n_lines[i] == left:
                hit["lines_equal_left"] += 1
            if bits[i] == 0:
                bits[i] += 2
                left -= 2 * n_lines[i]
                running[i] -= 12.0
                if left < 0:
                    hit["two_bit_negative"] += 1
            else:
                bits[i] += 1
                left -= n_lines[i]
                running[i] -= 6.0
            if left == 0:
                hit["left_zero_after_grant"] += 1
        else:
            hit["retired_full" if not bits[i] < max_mant else "retired_no_bits"] += 1
            running[i] = _DEAD
            retired += 1
            if retired == n_bands:
                hit["all_retired"] = 1
                break
    if int(left) < 0:
        hit["negative_out"] = 1
    return bits, int(left), hit


# ------------------------------------------------------------------------------------------------ streams
N_STREAMS, STREAM_BLOCKS = 8, 300                            # the scan refills its ring of item ids at items 136 and 264
STREAM_CONFIGS = [(1024, 1024, False, 2.86), (1024, 1024, True, 2.86), (128, 128, False, 2.86), (128, 128, True, 2.86)]


def stream_cases(cfg):
    """8 streams of 300 consecutive blocks whose SMRs cycle through the families; reservoir [8] to start from"""
    def make():
        lay = layout(cfg)
        rng = np.random.default_rng([77, cfg[0], cfg[1], int(cfg[2])])
        n = N_STREAMS * STREAM_BLOCKS
        fam = np.arange(n) % len(FAMILIES)
        vectors = np.stack([family_smr(FAMILIES[f], lay["n_tot"], lay["nb"], rng) for f in fam])
        lines, osc = make_lines(cfg, n, rng)
        out = _assemble(cfg, fam, vectors, lines, osc)
        out["reservoir"] = np.concatenate([[0, -5000, 40000, 10 ** 6], rng.integers(-3000, 30000, 4)]).astype(np.int64)
        return out
    return _cached(("streams",) + tuple(cfg), make)


def stream_reference(cfg, streams=range(N_STREAMS), saved_of=None):
    """the oracle block after block, reservoir = int(left) carried forward (+ saved_of(block index, bits [ns][nb], scale
    factors, mantissas) -> (bits saved, table ids [ns]) where the caller prices Huffman tables) -> bit_alloc, scale_factor,
    mantissa, trace [block] and table for the blocks of `streams`, in stream order"""
    lay, c = layout(cfg), stream_cases(cfg)
    nb, ns = lay["nb"], lay["ns"]
    idx = np.concatenate([np.arange(s * STREAM_BLOCKS, (s + 1) * STREAM_BLOCKS) for s in streams])
    bits = np.empty((len(idx), lay["n_tot"]), np.int64)
    trace = np.empty(len(idx), np.int64)
    table = np.full((len(idx), ns), 15, np.int64)
    sf = mant = None
    if saved_of is not None:
        sf = np.empty((len(idx), ns, nb), np.int64)
        mant = np.empty((len(idx), ns, lay["half"]), np.int64)
    for j, i in enumerate(idx):
        if i % STREAM_BLOCKS == 0:
            res = int(c["reservoir"][i // STREAM_BLOCKS])
        bi, left = BitAlloc(budget_of(cfg, res), MAX_MANT, lay["n_tot"], lay["n_lines"], c["vectors"][i].copy())
        bits[j] = bi.astype(np.int64)
        res = int(left)
        if saved_of is not None:
            sf[j:j + 1], mant[j:j + 1] = _quantise(cfg, c["coded"][i:i + 1], bits[j:j + 1])
            saved, table[j] = saved_of(i, bits[j].reshape(ns, nb), sf[j], mant[j])
            res += int(saved)
        trace[j] = res
    if saved_of is None:
        sf, mant = _quantise(cfg, c["coded"][idx], bits)
    return dict(index=idx, bit_alloc=bits.reshape(len(idx), ns, nb), scale_factor=sf, mantissa=mant, trace=trace, table=table)
