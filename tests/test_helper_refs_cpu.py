"""
The references of tests/test_gpu_helper_probes.py (tests/helper_refs.py) held on the CPU, so that they are not the weak point:
the lane models composed as csrc/mrc_wave.hpp composes them reproduce sum, maximum and cumulative sum; the exact quantiser
restatement equals oracle/quantize.py on the golden inputs; the 80-digit and the long-double references agree; the tables the
device is compared with are the headers' own; and every input set holds the edge classes its test relies on.
"""
import os
from fractions import Fraction

import mpmath
import numpy as np

import helper_refs as R
from oracle import quantize


# ------------------------------------------------------------------------------------------------ lane models
def test_lane_moves_are_permutations_and_involutions():
    tags = R.wave_tags()
    for ctrl in R.DPP_SOURCE:
        once = R.dpp_move(ctrl, tags)
        assert np.array_equal(np.sort(once, axis=1), tags) and not np.array_equal(once, tags)
        assert np.array_equal(R.dpp_move(ctrl, once), tags)
        assert np.array_equal(once // 16, tags // 16)                  # a DPP move stays inside its 16-lane row
    assert np.array_equal(R.dpp_move(0x141, tags)[0, :8], np.arange(8)[::-1])
    for dist in (16, 32):
        x, y = R.rows_swap(dist, tags, tags + 10000)
        both = np.sort(np.concatenate([x, y], axis=1), axis=1)
        assert np.array_equal(both, np.sort(np.concatenate([tags, tags + 10000], axis=1), axis=1))
        low = (R.LANE & dist) == 0
        assert np.array_equal(x[:, low], tags[:, low]) and np.array_equal(y[:, ~low], tags[:, ~low] + 10000)
        assert np.array_equal(x[:, ~low], tags[:, low] + 10000) and np.array_equal(y[:, low], tags[:, ~low])


def test_reductions_composed_as_the_header_composes_them():
    v = R.exact_sum_doubles(1)
    rows = v.reshape(-1, 4, 16)
    assert np.array_equal(R.row_reduce(v, np.add), np.repeat(rows.sum(axis=2), 16, axis=1))
    assert np.array_equal(R.row_reduce(v, np.fmax), np.repeat(rows.max(axis=2), 16, axis=1))
    assert np.array_equal(R.wave_allreduce(v, np.add), np.repeat(v.sum(axis=1, keepdims=True), 64, axis=1))
    p = R.max_permutations(2)
    assert np.array_equal(np.argmax(p[:64], axis=1), np.arange(64))
    assert np.array_equal(R.wave_allreduce(p, np.fmax), np.repeat(p.max(axis=1, keepdims=True), 64, axis=1))
    a, b, c, d = (R.exact_sum_doubles(s) for s in (3, 4, 5, 6))
    want4 = np.concatenate([np.repeat(t.sum(axis=1, keepdims=True), 16, axis=1) for t in (a, b, c, d)], axis=1)
    assert np.array_equal(R.wave_fold4(a, b, c, d, np.add), want4)
    want2 = np.concatenate([np.repeat(t.sum(axis=1, keepdims=True), 32, axis=1) for t in (a, b)], axis=1)
    assert np.array_equal(R.wave_fold2(a, b, np.add), want2)
    v8 = R.exact_sum_doubles(7, (R.N_WAVES, 8, 64))
    assert np.array_equal(R.wave_sum_block8(v8), np.repeat(v8.sum(axis=2, keepdims=True), 64, axis=2))


def test_scan_model_is_the_cumulative_sum():
    steps = R.scan_steps()
    assert np.array_equal(R.wave_incl_scan(steps), np.cumsum(steps, axis=1))
    for k in (15, 16, 31, 32, 47, 48):                                 # the row boundaries
        assert list(R.wave_incl_scan(steps)[k]) == [0] * k + [1] * (64 - k)
    v = R.exact_sum_ints(8)
    assert np.array_equal(R.wave_incl_scan(v), np.cumsum(v, axis=1))
    # ... and a model without one of the row broadcasts is NOT (the test's reference can tell the mutation)
    w = steps
    for k in (1, 2, 4, 8):
        w = w + R.row_shr(k, w)
    assert not np.array_equal(w + R.row_bcast(15, (1, 3), w), np.cumsum(steps, axis=1))


# ------------------------------------------------------------------------------------------------ quantiser
def test_exact_quantiser_equals_the_oracle_on_the_golden_inputs(golden_dir):
    g = np.load(os.path.join(golden_dir, "quantize.npz"), allow_pickle=False)
    vals = [float(v) for v in g["vals"]]
    for nb, want in zip(g["nbits_cases"], g["quant_out"]):
        nb = int(nb)
        got = [R.mag_code_exact(abs(v), nb) + ((1 << (nb - 1)) if v < 0 else 0) for v in vals]
        assert got == list(want) == [quantize.QuantizeUniform(v, nb) for v in vals]
    for (s, m), want in zip(g["sf_cases"], g["sf_out"]):
        assert [R.scale_factor_exact(v, int(s), int(m)) for v in vals] == list(want)
    for (sc, sb, mb), want in zip(g["mant_cases"], g["vmant_out"]):
        assert [R.mantissa_exact(v, int(sc), int(sb), int(mb)) for v in vals] == [int(w) for w in want]


def test_quantiser_edges_are_edges():
    for r in R.N_BITS_ALL:
        top = (1 << (r - 1)) - 1
        assert {1, top} <= set(R.edge_codes(r)) and (r < 4 or 1 << (r - 2) in R.edge_codes(r))
        for c in R.edge_codes(r):
            e = R.code_edge(c, r)
            assert (Fraction((1 << r) - 1) * e + 1) / 2 == c
            m = R.fl(e)
            codes = [R.mag_code_exact(v, r) for v in (np.nextafter(np.nextafter(m, 0.0), 0.0), np.nextafter(np.nextafter(m, 2.0), 2.0))
                     if v < 1.0]
            assert codes[0] in (c - 1, c) and codes[-1] in (c - 1, c, c + 1)
            if r <= 30 and len(codes) == 2 and c < top:                # the five doubles straddle the step (one ulp of the
                assert codes == [c - 1, c], (r, c, codes)              # magnitude moves the sum by less than one unit)
        mags = R.edge_magnitudes(r)
        assert 0.0 in mags and 1.0 in mags and np.nextafter(1.0, 0.0) in mags
        assert R.mag_code_exact(1.0, r) == top and R.mag_code_exact(0.0, r) == 0
    mags, bits = R.mag_code_inputs()
    assert len(mags) == len(bits) <= R.MAX_SET and set(bits) == set(R.N_BITS_ALL)
    x, sc, sb, mb = R.scale_mant_inputs()
    assert len(x) <= R.MAX_SET and (x < 0).any() and (x == 1.0).any() and (x == 0.0).any()
    combos = set(zip(sc.tolist(), sb.tolist(), mb.tolist()))
    assert combos == {(k, s, m) for s in range(1, 5) for m in range(2, 17) for k in range(1 << s)}


# ------------------------------------------------------------------------------------------------ math references
def test_long_double_and_80_digit_references_agree():
    assert np.finfo(R.LD).nmant >= 63
    rng = np.random.default_rng(5)
    x = np.concatenate([R.atan_inputs()[::257], [0.5, 1.0, 200.0]])
    for v, ld in zip(x[x > 0], np.arctan(x[x > 0].astype(R.LD))):
        assert R.ulp_err_mp(float(ld), mpmath.atan(R.mp_of(v))) <= 0.5 + 2.0 ** -9
        assert abs(mpmath.mpf(float(ld)) + mpmath.mpf(float(ld - R.LD(float(ld)))) - mpmath.atan(R.mp_of(v))) \
            <= mpmath.atan(R.mp_of(v)) * 2.0 ** -62
    x = R.log10_inputs()[::509]
    for v, ld in zip(x, np.log10(x.astype(R.LD))):
        hi = float(ld)
        assert abs(mpmath.mpf(hi) + mpmath.mpf(float(ld - R.LD(hi))) - mpmath.log10(R.mp_of(v))) <= \
            max(abs(mpmath.log10(R.mp_of(v))) * 2.0 ** -62, mpmath.mpf(2) ** -70)
    sT, u = R.exp2_tab_inputs()
    for T in (64, 256):
        ld, g = R.exp2_tab_exact_ld(sT, u, T)
        assert np.abs(g).max() <= 0.5
        for i in rng.integers(0, len(sT), 200):
            want = R.exp2_tab_exact_mp(sT[i], u[i], T)
            assert abs(mpmath.mpf(float(ld[i])) + mpmath.mpf(float(ld[i] - R.LD(float(ld[i])))) - want) <= want * 2.0 ** -61
    x = R.rcp_inputs()[::997]
    x = x[x < 2.0 ** 900]                                               # (a long double's two halves as doubles: both normal)
    for v, ld in zip(x, 1 / x.astype(R.LD)):
        hi = float(ld)
        assert abs(mpmath.mpf(hi) + mpmath.mpf(float(ld - R.LD(hi))) - 1 / R.mp_of(v)) <= 2.0 ** -62 / R.mp_of(v)
    # the two error measures on one made-up result
    assert float(R.ulp_err_mp(1.0 + 2.0 ** -52, 1)) == 1.0 and float(R.ulp_err_ld(np.array([1.0 + 2.0 ** -52]), R.LD(1))[0]) == 1.0
    assert R.ulp_err_mp(0.75, mpmath.mpf(1) - mpmath.mpf(2) ** -60) == (mpmath.mpf(1) / 4 - mpmath.mpf(2) ** -60) * 2 ** 53
    assert float(R.ulp_of(R.LD(1.5))) == 2.0 ** -52 and float(R.ulp_of(R.LD(0.75))) == 2.0 ** -53


def test_two_prod_is_exact():
    sT, u = R.exp2_tab_inputs()
    p, e = R.two_prod(sT, u)
    for i in range(0, len(sT), 211):
        assert Fraction(float(p[i])) + Fraction(float(e[i])) == Fraction(float(sT[i])) * Fraction(float(u[i]))


def test_tables_the_device_is_compared_with():
    assert np.array_equal(R.exp2_table(64), R.header_doubles("mrc_smr_math.hpp", "kExp2Tab"))
    assert np.array_equal(R.exp2_table(256), R.header_doubles("mrc_smr_sweep.hpp", "kExp2Tab256"))
    assert np.array_equal(R.exp2_table(256)[::4], R.exp2_table(64))
    assert np.array_equal(R.atan_q_fit(), R.header_doubles("mrc_smr_math.hpp", "kAtanQ"))
    words = R.log_table_words()
    assert words.shape == (128,) and not words[3::4].any()
    for j in range(32):                                                # {1/c rounded, log10 c = hi + lo}, c ~ 1/2 + (j + 1/2)/64
        inv, hi, lo = (mpmath.mpf(float(w)) for w in words[4 * j:4 * j + 3])
        assert float(inv) == float(1 / (mpmath.mpf(1) / 2 + (mpmath.mpf(j) + mpmath.mpf(1) / 2) / 64))
        assert abs(hi + lo + mpmath.log10(inv)) < mpmath.mpf(2) ** -105


# ------------------------------------------------------------------------------------------------ input sets
def test_wave_input_sets_hold_their_edge_classes():
    assert R.N_WAVES % 12 == 0 and R.N_WAVES >= 64
    tags = R.wave_tags()
    assert tags.shape == (R.N_WAVES, 64) and len(np.unique(tags)) == tags.size
    for make in (R.max_permutations, R.all_negative_permutations):
        p = make(9)
        assert np.array_equal(np.argmax(p[:64], axis=1), np.arange(64))
        assert all(len(set(row)) == 64 for row in p) and (p < 0).any()
    assert (R.all_negative_permutations(9) < 0).all()
    z = R.signed_zero_waves()
    assert all(np.signbit(z[w]).sum() == 63 and not np.signbit(z[w, w]) for w in range(64))
    assert np.signbit(z[64]).all() and not np.signbit(z[65]).any() and (z[66:].max(axis=1) == 0).all()
    for s in (R.exact_sum_doubles(1), R.exact_sum_doubles(1, (R.N_WAVES, 17, 64))):
        assert np.array_equal(s, np.rint(s)) and np.abs(s).max() * 64 * 17 < 2.0 ** 53
    assert np.abs(R.exact_sum_ints(1)).max() * 64 < 2 ** 31
    steps = R.scan_steps()
    assert np.array_equal(steps[:64], np.eye(64, dtype=np.int64))
    o = R.ordered_doubles()
    assert (np.diff(o) >= 0).all() and o[0] == -np.inf and o[-1] == np.inf and o[-2] == np.finfo(float).max
    zero = np.flatnonzero(o == 0)
    assert list(np.signbit(o[zero])) == [True, False]
    tiny = np.finfo(float).tiny
    assert ((o > 0) & (o < tiny)).sum() >= 2 and ((o < 0) & (o > -tiny)).sum() >= 2 and (o < -1e299).sum() >= 3
    assert {np.nextafter(1.0, 0.0), 1.0, np.nextafter(1.0, 2.0)} <= set(o)
    b, g = R.xcd_inputs()
    assert len(b) <= R.MAX_SET and set(g) == set(R.XCD_GRIDS) and all((b[g == k] == np.arange(k)).all() for k in R.XCD_GRIDS)


def test_math_input_sets_hold_their_edge_classes():
    x = R.rcp_inputs()
    m, e = np.frexp(x)
    assert len(x) <= R.MAX_SET and (x >= np.finfo(float).tiny).all() and np.isfinite(x).all()
    e = e - 1
    assert set(range(R.RCP_EXP_LO, R.RCP_EXP_HI + 1)) <= set(e) and {-1022, 1023} <= set(e)
    assert R.RCP_EXP_LO == int(np.floor(np.log2(1e-12)))
    for k in (R.RCP_EXP_LO, 0, 1023, -1022):
        mk = 2 * m[e == k]
        assert len(mk) >= (1 << 12) + (1 << 10) + 8
        assert {1.0, np.nextafter(1.0, 2.0), np.nextafter(2.0, 1.0)} <= set(mk)
        assert set(1.0 + np.arange(1 << 12) / (1 << 12)) <= set(mk)
    a2, t = R.line_ratio_inputs()
    assert (a2 == 0).any() and np.isinf(t).sum() == len(t) // 2 and a2.max() > 1e29 and (t[np.isfinite(t)] >= 1e-12).all()
    f = R.exp2_poly_inputs()
    assert len(f) == R.MAX_SET and {-0.5, 0.5, 0.0} <= set(f[:3]) and np.abs(f).max() == 0.5
    sT, u = R.exp2_tab_inputs()
    p, e2 = R.two_prod(sT, u)
    assert len(sT) <= R.MAX_SET and np.abs(p).max() < 16000
    exact = e2 == 0
    assert (exact & (p == 0)).sum() >= 128 and (sT[p == 0] != 0).any() and (u[p == 0] != 0).any()
    assert (exact & (p == np.rint(p)) & (p != 0)).sum() >= 1000
    ties = exact & (np.abs(p - np.trunc(p)) == 0.5)
    assert ties.sum() >= 1000 and (np.trunc(p[ties]) % 2 == 0).any() and (np.trunc(p[ties]) % 2 == 1).any()
    g = (p - np.rint(p)) + e2                                           # just beside an integer / a tie: |distance| tiny, not 0
    near_int = (np.abs(g) < 1e-9) & (g != 0)
    near_tie = (np.abs(np.abs(g) - 0.5) < 1e-9) & (np.abs(g) != 0.5)
    assert near_int.sum() >= 1000 and near_tie.sum() >= 1000
    hi, lo = R.exp2_dd_inputs()
    assert len(hi) <= R.MAX_SET and np.abs(hi).max() < 1000 and np.abs(lo).max() < 2.0 ** -40
    fr = (hi - np.rint(hi)).astype(R.LD) + lo.astype(R.LD)
    assert np.abs(fr).max() <= 0.5 and (np.abs(hi - np.rint(hi)) == 0.5).sum() >= 1000 and (hi == np.rint(hi)).sum() >= 1000
    (h, l), (xh, xl), kinds = R.dd_inputs()
    assert len(h) <= R.MAX_SET and set(kinds) == {0, 1, 2, 3, 4}
    for a, b in ((h, l), (xh, xl)):
        assert (np.abs(b) <= np.ldexp(0.5, np.frexp(a)[1] - 53)).all() and np.array_equal(a + b, a)
    assert (np.abs(xh[kinds == 1]) < np.abs(h[kinds == 1]) * 2.0 ** -59).all()
    assert (np.abs(h[kinds == 2] + xh[kinds == 2]) <= np.abs(h[kinds == 2]) * 2.0 ** -50).all()
    assert np.array_equal(xh[kinds == 3], -h[kinds == 3]) and np.array_equal(xl[kinds == 3], -l[kinds == 3])
    r = -xh[kinds == 4] / h[kinds == 4]
    assert (r >= 0.5 - 1e-9).all() and (r <= 2 + 1e-9).all() and (np.abs(r - 1) < 0.01).sum() >= 10
    x = R.atan_inputs()
    assert len(x) <= R.MAX_SET and x[0] == 0 and (x >= 0).all() and x.max() == 200.0
    assert ((x > 0) & (x < np.finfo(float).tiny)).sum() >= 2 and ((x > 0) & (x <= 1)).sum() >= (1 << 16) - (1 << 12) - 1
    assert {np.nextafter(1.0, 0.0), 1.0, np.nextafter(1.0, 2.0)} <= set(x) and (x > 1).sum() >= 3000
    x = R.log10_inputs()
    assert len(x) == R.MAX_SET and x.min() < 1e-290 and x.max() > 1e290
    assert (np.abs(x - 1) <= 0.01).sum() >= 1 << 15 and (np.abs(x - 1) <= 1e-5).sum() >= 1 << 14
    e = R.SPL_EDGES
    assert (e == 0).any() and np.isnan(e).any() and (e == np.inf).any() and (e < 0).any() and np.finfo(float).tiny in e
    assert ((e > 0) & (e < np.finfo(float).tiny)).any()
