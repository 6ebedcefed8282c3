"""
GPU tests of the kernels' __device__ helpers one by one: the cross-lane primitives of csrc/mrc_wave.hpp, the math helpers of
csrc/mrc_smr_math.hpp and the quantiser templates at the top of csrc/mrc_device.hpp, each called UNCHANGED by a probe kernel
(csrc/mrc_kernels_probe.hip through mrc_dev_helper_probe) on inputs made here, against the references of
tests/helper_refs.py (held on the CPU by tests/test_helper_refs_cpu.py).

Lane maps, sums of exactly summable values, maxima, scans and every integer are compared bit for bit.  A math helper is held to
the bound its own comment (or DESIGN.md) states; where the comments give pieces only, the docstring of the test derives the
total.  A test that measures an error prints the maximum and the input that produced it (pytest -s shows them).
"""
import os
import re
import subprocess
from fractions import Fraction

import mpmath
import numpy as np
import pytest

import helper_refs as R

pytestmark = pytest.mark.gpu

# (threads per workgroup, workgroups per launch): 64 and 256 threads, 1 and 3 workgroups
CONFIGS = [(64, 1), (64, 3), (256, 1), (256, 3)]
MATH_THREADS = (128, 256)            # the short-block masking kernel's size, the long one's


def _words(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float64:
        return a.view(np.int64)
    return a.astype(np.int64)


class Dev:
    def __init__(self, torch, h):
        self.torch, self.h = torch, h

    def run(self, name, ins, threads=64):
        """ins: up to three arrays [n] or [words][n]; returns the output words as uint64 [words][n]"""
        from mrcaudiocodec_amd import _lib
        pid, win, wout = _lib.PROBES[name]
        torch = self.torch
        ins = [np.atleast_2d(_words(a)) for a in ins]
        assert [len(a) for a in ins] == [w for w in win if w], (name, [a.shape for a in ins])
        n = ins[0].shape[1] if ins else None
        t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in ins]
        ptr = [x.data_ptr() for x in t] + [None] * (3 - len(t))
        return self._launch(pid, ptr, wout, n, threads)

    def _launch(self, pid, ptr, wout, n, threads):
        torch = self.torch
        out = torch.full((wout * n,), -0x0123456789ABCDEF, dtype=torch.int64, device="cuda")
        self.h.dev_helper_probe(pid, ptr[0], ptr[1], ptr[2], out.data_ptr(), wout * n, n, threads)
        torch.cuda.synchronize()
        return out.cpu().numpy().view(np.uint64).reshape(wout, n)

    def run_n(self, name, n, threads=64):
        """a probe without inputs"""
        from mrcaudiocodec_amd import _lib
        pid, _, wout = _lib.PROBES[name]
        return self._launch(pid, [None] * 3, wout, n, threads)

    def run_waves(self, name, ins, threads, groups):
        """ins: arrays [waves][64] or [words][waves][64]; launches of `groups` workgroups of `threads` threads, every wave
        with its own data; returns uint64 [words][waves][64]"""
        ins = [_words(a) for a in ins]
        ins = [a[None] if a.ndim == 2 else a for a in ins]
        nw, per = ins[0].shape[1], (threads // 64) * groups
        assert nw % per == 0
        outs = []
        for w in range(0, nw, per):
            part = [a[:, w:w + per].reshape(a.shape[0], -1) for a in ins]
            o = self.run(name, part, threads)
            outs.append(o.reshape(o.shape[0], per, 64))
        return np.concatenate(outs, axis=1)


@pytest.fixture(scope="module")
def dev():
    torch = pytest.importorskip("torch")
    from mrcaudiocodec_amd import Handle
    h = Handle(device_id=0)
    yield Dev(torch, h)
    h.close()


def _f64(w):
    return np.ascontiguousarray(w).view(np.float64)


def _i64(w):
    return np.ascontiguousarray(w).view(np.int64)


def _bits(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64)).view(np.uint64)


def _same_bits(got_words, want_doubles, what):
    bad = np.flatnonzero((got_words != _bits(want_doubles)).ravel())
    assert bad.size == 0, "%s: %d differ, first at %d: got %r, want %r" % (
        what, bad.size, bad[0], _f64(got_words).ravel()[bad[0]], np.asarray(want_doubles).ravel()[bad[0]])


def _report(what, err, unit, bound, where):
    where = re.sub(r"np\.float64\(([^)]*)\)", r"\1", where)
    print("\n[helper-probe] %-34s max %.6g %s (bound %.6g) at %s" % (what, err, unit, bound, where))


# ------------------------------------------------------------------------------------------------ the entry point
def test_entry_point_refuses_bad_arguments(dev):
    from mrcaudiocodec_amd import MrcError, _lib
    torch = dev.torch
    buf = torch.zeros(1024, dtype=torch.int64, device="cuda")
    p = buf.data_ptr()
    ok = dict(probe=_lib.PROBES["SCAN_I32"][0], in0=p, in1=None, in2=None, out=p + 4096, out_words=64, n=64, threads=64)
    dev.h.dev_helper_probe(**ok)
    torch.cuda.synchronize()
    for change in (dict(probe=0), dict(probe=999), dict(n=0), dict(n=-1), dict(n=65537), dict(threads=32), dict(threads=192),
                   dict(threads=512), dict(threads=0), dict(in0=None), dict(out=None), dict(out_words=63)):
        with pytest.raises(MrcError) as e:
            dev.h.dev_helper_probe(**dict(ok, **change))
        assert e.value.code == _lib.MRC_ERR_INVALID, change
    with pytest.raises(MrcError):                                       # a second input the probe reads
        dev.h.dev_helper_probe(**dict(ok, probe=_lib.PROBES["XCD"][0]))


@pytest.mark.parametrize("threads", [64, 128, 256])
def test_ragged_counts_write_only_their_elements(dev, threads):
    """n that is no multiple of the wave: lanes past the end compute on the last element and store nothing"""
    torch = dev.torch
    from mrcaudiocodec_amd import _lib
    for n in (1, 63, 65, 257, 1000):
        v = np.arange(1, n + 1, dtype=np.int64)
        src = torch.from_numpy(v).cuda()
        out = torch.full((n + 512,), -7, dtype=torch.int64, device="cuda")
        dev.h.dev_helper_probe(_lib.PROBES["SCAN_I32"][0], src.data_ptr(), None, None, out.data_ptr(), n, n, threads)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[n:] == -7).all()
        pad = np.concatenate([v, np.full((-n) % 64, n)]).reshape(-1, 64)
        assert np.array_equal(got[:n], np.cumsum(pad, axis=1).ravel()[:n])


# ------------------------------------------------------------------------------------------------ wave primitives
@pytest.mark.parametrize("threads,groups", CONFIGS)
def test_lane_moves(dev, threads, groups):
    """dpp_move for 0xB1, 0x4E, 0x141, 0x128 and rows_swap<16>, <32> on int, unsigned and double: the lane maps the comments
    of mrc_wave.hpp state, bit for bit, with lane + 64 wave as the tag (in both halves of a double)"""
    tag = R.wave_tags()
    other = tag + 100000
    cases = {"MOVES_I32": (-tag - 1, -other - 1), "MOVES_U32": (tag | 0x80000000, other | 0x80000000),
             "MOVES_F64": ((tag << 32) | tag, (other << 32) | other)}
    for name, (a, b) in cases.items():
        got = _i64(dev.run_waves(name, [a, b], threads, groups))
        want = [R.dpp_move(c, a) for c in (0xB1, 0x4E, 0x141, 0x128)] + list(R.rows_swap(16, a, b)) + list(R.rows_swap(32, a, b))
        for k, w in enumerate(want):
            assert np.array_equal(got[k], w), (name, k)


@pytest.mark.parametrize("threads,groups", CONFIGS)
def test_wave_sums(dev, threads, groups):
    """wave_sum, row_reduce(+), wave_sum_i, row_reduce on ints, wave_sum_block<8>, wave_sum_all<9 / 16 / 17> (the far field's
    instantiations) on integer-valued inputs: every order of summation is exact, so the totals equal Python's sum"""
    v = R.exact_sum_doubles(41)
    got = dev.run_waves("SUM_F64", [v], threads, groups)
    total = np.array([[float(sum(int(x) for x in row))] * 64 for row in v])
    _same_bits(got[0], total, "wave_sum")
    _same_bits(got[1], np.repeat(v.reshape(-1, 4, 16).sum(axis=2), 16, axis=1), "row_reduce(+)")
    iv = R.exact_sum_ints(42)
    gi = _i64(dev.run_waves("REDUCE_I32", [iv], threads, groups))
    assert np.array_equal(gi[0], np.repeat(iv.sum(axis=1, keepdims=True), 64, axis=1))
    assert np.array_equal(gi[1], np.repeat(iv.max(axis=1, keepdims=True), 64, axis=1))
    assert np.array_equal(gi[2], np.repeat(iv.reshape(-1, 4, 16).sum(axis=2), 16, axis=1))
    assert np.array_equal(gi[3], np.repeat(iv.reshape(-1, 4, 16).max(axis=2), 16, axis=1))
    for name, n in (("SUM_BLOCK8", 8), ("SUM_ALL9", 9), ("SUM_ALL16", 16), ("SUM_ALL17", 17)):
        vn = R.exact_sum_doubles(43 + n, (n, R.N_WAVES, 64))
        gn = dev.run_waves(name, [vn], threads, groups)
        _same_bits(gn, np.repeat(vn.sum(axis=2, keepdims=True), 64, axis=2), name)


@pytest.mark.parametrize("threads,groups", CONFIGS)
def test_wave_maxima(dev, threads, groups):
    """wave_max, wave_max_i and row_max on permutations with the maximum in each of the 64 lanes in turn, negative values
    included; -0.0 against +0.0 and one NaN lane for wave_max (fmax drops it; none for row_max / max_raw)"""
    for p in (R.max_permutations(51), R.all_negative_permutations(52)):
        _same_bits(dev.run_waves("MAX_F64", [p], threads, groups)[0], np.repeat(p.max(axis=1, keepdims=True), 64, axis=1), "wave_max")
        _same_bits(dev.run_waves("ROW_MAX", [p], threads, groups)[0], np.repeat(p.reshape(-1, 4, 16).max(axis=2), 16, axis=1), "row_max")
        ip = np.rint(p * 4).astype(np.int64)
        gi = _i64(dev.run_waves("REDUCE_I32", [ip], threads, groups))
        assert np.array_equal(gi[1], np.repeat(ip.max(axis=1, keepdims=True), 64, axis=1))
    p = R.max_permutations(53)
    nan_at = (np.arange(R.N_WAVES) * 5 + 3) % 64
    nan_at = np.where(nan_at == np.argmax(p, axis=1), (nan_at + 1) % 64, nan_at)
    p[np.arange(R.N_WAVES), nan_at] = np.nan
    _same_bits(dev.run_waves("MAX_F64", [p], threads, groups)[0], np.repeat(np.nanmax(p, axis=1, keepdims=True), 64, axis=1),
               "wave_max with a NaN lane")
    z = R.signed_zero_waves()
    got = _f64(dev.run_waves("MAX_F64", [z], threads, groups)[0])
    assert (got == 0).all()
    assert not np.signbit(got[65]).any() and np.signbit(got[64]).all() and np.signbit(got[66:]).all()
    print("\n[helper-probe] wave_max of 63 x -0.0 and one +0.0: +0.0 in %d of 64 waves" % int((~np.signbit(got[:64, 0])).sum()))


@pytest.mark.parametrize("threads,groups", CONFIGS)
def test_wave_folds(dev, threads, groups):
    """wave_fold4 (double fmax; the packed-unsigned add of the chain) leaves value r in every lane of row r; wave_fold2 leaves a
    in lanes 0-31 and b in lanes 32-63"""
    rng = np.random.default_rng(61)
    four = np.stack([R.max_permutations(62 + k) * (k + 1) for k in range(4)])
    four[1] -= 500.0                                                   # one value all negative
    four[2, 64] = R.signed_zero_waves()[3]                             # -0.0 against +0.0
    got = _f64(dev.run_waves("FOLD4_F64", [four], threads, groups)[0])
    want = np.concatenate([np.repeat(four[r].max(axis=1, keepdims=True), 16, axis=1) for r in range(4)], axis=1)
    assert np.array_equal(got, want)
    packed = rng.integers(0, 256, (4, R.N_WAVES, 64)) | (rng.integers(0, 256, (4, R.N_WAVES, 64)) << 16)
    gu = _i64(dev.run_waves("FOLD4_U32", [packed], threads, groups)[0])
    assert np.array_equal(gu, np.concatenate([np.repeat(packed[r].sum(axis=1, keepdims=True), 16, axis=1) for r in range(4)], axis=1))
    ints = np.stack([R.exact_sum_ints(63), R.exact_sum_ints(64)])
    dbls = np.stack([R.exact_sum_doubles(65), R.exact_sum_doubles(66)])
    g2 = dev.run_waves("FOLD2", [ints, dbls], threads, groups)
    half = lambda t: np.concatenate([np.repeat(t[r].sum(axis=1, keepdims=True), 32, axis=1) for r in range(2)], axis=1)
    assert np.array_equal(_i64(g2[0]), half(ints))
    _same_bits(g2[1], half(dbls), "wave_fold2 of doubles")


@pytest.mark.parametrize("threads,groups", CONFIGS)
def test_wave_scan(dev, threads, groups):
    """wave_incl_scan for int and double: a single 1 at lane k gives the step function at k, for every k (each lane's reach
    across the row boundaries 15/16, 31/32, 47/48); random exact-integer inputs equal np.cumsum"""
    steps = R.scan_steps()
    gi = _i64(dev.run_waves("SCAN_I32", [steps], threads, groups)[0])
    gd = _f64(dev.run_waves("SCAN_F64", [steps.astype(np.float64)], threads, groups)[0])
    for k in range(64):
        want = [0] * k + [1] * (64 - k)
        assert list(gi[k]) == want and list(gd[k]) == want, k
    assert np.array_equal(gi, np.cumsum(steps, axis=1))
    iv, dv = R.exact_sum_ints(71), R.exact_sum_doubles(72)
    assert np.array_equal(_i64(dev.run_waves("SCAN_I32", [iv], threads, groups)[0]), np.cumsum(iv, axis=1))
    _same_bits(dev.run_waves("SCAN_F64", [dv], threads, groups)[0], np.cumsum(dv, axis=1), "wave_incl_scan of doubles")


@pytest.mark.parametrize("threads", [64, 256])
def test_order_key(dev, threads):
    """order_key is strictly increasing (as unsigned 64-bit values) along a sorted list from -inf over the denormals and both
    zeros to +inf, and order_value returns the same bits"""
    v = R.ordered_doubles()
    got = dev.run("ORDER_KEY", [v], threads)
    keys = [int(k) for k in got[0]]
    assert all(a < b for a, b in zip(keys, keys[1:]))
    assert np.array_equal(got[1], _bits(v))


@pytest.mark.parametrize("threads", [64, 256])
def test_xcd_contiguous(dev, threads):
    """xcd_contiguous(b, g) for all b < g: a bijection onto [0, g), and the blocks with b % 8 == x get one contiguous ascending
    range, the ranges of x = 0..7 behind each other"""
    b, g = R.xcd_inputs()
    got = _i64(dev.run("XCD", [b, g], threads)[0])
    for grid in R.XCD_GRIDS:
        u = got[g == grid]
        assert sorted(u) == list(range(grid)), grid
        start = 0
        for x in range(8):
            mine = u[x::8]
            assert list(mine) == list(range(start, start + len(mine))), (grid, x)
            start += len(mine)


# ------------------------------------------------------------------------------------------------ reciprocal
@pytest.mark.parametrize("threads", MATH_THREADS)
def test_reciprocal(dev, threads):
    """The bare hardware reciprocal (__builtin_amdgcn_rcp) on positive normal doubles: relative error <= 2^-13, what recip_nr's
    two Newton steps need for their 2^-52 and what implies kRcpRel = 2^-12 of the bound pass (mrc_smr_body.hpp, DESIGN.md
    section 4); recip_nr on the same set: <= 2^-52 while 1/x is a normal number (x <= 2^1022).  Beyond that 1/x is subnormal,
    on a grid of 2^-1074 -- coarser than 2^-52 relative, for any result: there recip_nr's last step rounds a value within
    2^-52 relative (< 2^-1074) of 1/x to that grid, so it is within 1.5 x 2^-1074 of 1/x (the comment of recip_nr says so; the
    masking kernels' thresholds end far below 2^1022 or at +inf, which line_ratio takes care of)."""
    x = R.rcp_inputs()
    got = _f64(dev.run("RCP", [x], threads))
    exact = 1 / x.astype(R.LD)
    for k, (what, bound) in enumerate((("rcp", 2.0 ** -13), ("recip_nr", 2.0 ** -52))):
        normal = x <= 2.0 ** 1022
        sel = np.flatnonzero(normal) if k == 1 else np.arange(len(x))
        err, i, gap = R.worst_case(R.rel_err_ld(got[k][sel], exact[sel]), lambda j: 1 / R.mp_of(x[sel[j]]), got[k][sel], "rel")
        _report(what + " (relative)", err, "= 2^%.2f" % np.log2(max(err, 1e-300)), bound, "x = %s" % float(x[sel[i]]).hex())
        assert err <= bound and gap <= 2.0 ** -60
        if k == 1:
            sub = np.flatnonzero(~normal)
            worst = max(abs(R.mp_of(got[1][j]) - 1 / R.mp_of(x[j])) for j in sub) * mpmath.mpf(2) ** 1074
            _report("recip_nr, subnormal 1/x", float(worst), "x 2^-1074", 1.5, "x > 2^1022")
            assert worst <= 1.5
    # per exponent class, for the record: the bare estimate over what t_ub can hold and at the extremes
    e = np.frexp(x)[1] - 1
    rel = R.rel_err_ld(got[0], exact)
    for lo, hi in ((R.RCP_EXP_LO, R.RCP_EXP_HI), (-1022, -1022), (1023, 1023)):
        m = (e >= lo) & (e <= hi)
        print("[helper-probe] rcp, exponents %d..%d: max relative error 2^%.2f" % (lo, hi, float(np.log2(rel[m].max()))))
    inf = _f64(dev.run("RCP", [np.array([np.inf, 1.0])], threads))
    assert inf[0][0] == 0.0 and not np.signbit(inf[0][0]) and inf[0][1] == 1.0


@pytest.mark.parametrize("threads", MATH_THREADS)
def test_line_ratio(dev, threads):
    """line_ratio(a2, +inf) == +0.0 exactly; otherwise fmax(fl(a2 recip_nr(t)), 0) is within (1 + 2^-52)(1 + 2^-53) - 1 of
    a2 / t: recip_nr's bound and the one product"""
    a2, t = R.line_ratio_inputs()
    got = _f64(dev.run("LINE_RATIO", [a2, t], threads)[0])
    at_inf = np.isinf(t)
    assert (got[at_inf] == 0).all() and not np.signbit(got[at_inf]).any()
    assert (got[a2 == 0] == 0).all() and not np.signbit(got[a2 == 0]).any()
    sel = np.flatnonzero(~at_inf & (a2 > 0))
    exact = a2[sel].astype(R.LD) / t[sel].astype(R.LD)
    bound = float((1 + mpmath.mpf(2) ** -52) * (1 + mpmath.mpf(2) ** -53) - 1)
    err, i, _ = R.worst_case(R.rel_err_ld(got[sel], exact), lambda j: R.mp_of(a2[sel[j]]) / R.mp_of(t[sel[j]]), got[sel], "rel")
    _report("line_ratio (relative)", err, "= 2^%.2f" % np.log2(err), bound, "a2 = %r, t = %r" % (a2[sel[i]], t[sel[i]]))
    assert err <= bound


# ------------------------------------------------------------------------------------------------ 2^x
@pytest.mark.parametrize("threads", MATH_THREADS)
def test_exp2_poly(dev, threads):
    """exp2_poly on [-0.5, 0.5], the ends, 0 and 2^16 points: relative error <= 2e-16 (its comment)"""
    f = R.exp2_poly_inputs()
    got = _f64(dev.run("EXP2_POLY", [f], threads)[0])
    err, i, _ = R.worst_case(R.rel_err_ld(got, np.exp2(f.astype(R.LD))), lambda j: mpmath.power(2, R.mp_of(f[j])), got, "rel")
    _report("exp2_poly (relative)", err, "", 2e-16, "f = %r" % f[i])
    assert err <= 2e-16
    assert got[2] == 1.0


def exp2_tab_bound(T):
    """The relative error of exp2_tab64<T> from the pieces its comment gives, u = 2^-53:
      * the table entry is correctly rounded: (1 + u);
      * p = 2^(g/T) for the EXACT g, as a Taylor polynomial in x = g ln2 / T, |x| <= ln2 / 2T: remainder |x|^d / d! e^|x|
        relative to the value (d = 6 for T = 64: 3.53e-17; d = 5 for T = 256: 3.80e-17);
      * the fma chain: its last step rounds a value in [2^(-1/2T), 2^(1/2T)] once -- half an ulp of 2^-53 from 1 up, of 2^-54
        below 1, so (1 + u) either way; the step before it rounds a value below 2^-6 (half an ulp 2^-60) that is then
        multiplied by |g| <= 1/2: 4.4e-19, the earlier ones below 1e-21; g itself is rounded once by its fma (the product has
        up to 106 bits): 2^-53 |g| ln2 / T <= 6.1e-19; ln2 / T as a double, times |g|: 6.1e-19, the higher coefficients below
        2e-21.  Together below 1.7e-18 absolute on a value >= 0.9946;
      * one product p * entry: (1 + u); ldexp is exact (results are normal numbers for |sT u| < 16000).
    Total (1 + u)^3 (1 + remainder + 1.7e-18 / 0.9946) - 1: 3.70e-16 for T = 64, 3.73e-16 for T = 256."""
    mp = mpmath.mp
    x = mp.ln2 / (2 * T)
    d = 6 if T == 64 else 5
    rem = x ** d / mpmath.factorial(d) * mpmath.exp(x)
    u = mpmath.mpf(2) ** -53
    return float((1 + u) ** 3 * (1 + rem + mpmath.mpf("1.7e-18") / mpmath.mpf("0.9946")) - 1)


@pytest.mark.parametrize("threads", MATH_THREADS)
def test_exp2_tab(dev, threads):
    """exp2_tab64<64>, <256> for |sT u| < 16000 -- exact integers, half-integers (the rint tie) and just beside them included --
    within exp2_tab_bound (derived there) of 2^(sT u / T) of the exact product, and exactly 1.0 at sT u == 0.
    exp2_tab_above<64>, <256> on the same inputs: never below the exact value, at most 2^(3/(2T)) (1 + 2^-52) times it."""
    sT, u = R.exp2_tab_inputs()
    got = _f64(dev.run("EXP2_TAB", [sT, u], threads))
    zero = (sT == 0) | (u == 0)
    assert zero.sum() >= 128 and (got[0][zero] == 1.0).all() and (got[1][zero] == 1.0).all()
    for k, T in enumerate((64, 256)):
        exact, _ = R.exp2_tab_exact_ld(sT, u, T)
        bound = exp2_tab_bound(T)
        err, i, gap = R.worst_case(R.rel_err_ld(got[k], exact), lambda j: R.exp2_tab_exact_mp(sT[j], u[j], T), got[k], "rel")
        _report("exp2_tab64<%d> (relative)" % T, err, "", bound, "sT = %r, u = %r" % (sT[i], u[i]))
        assert err <= bound and gap <= 2.0 ** -60
        above = got[2 + k].astype(R.LD) / exact
        top = float(mpmath.power(2, mpmath.mpf(3) / (2 * T)) * (1 + mpmath.mpf(2) ** -52))
        lo_i, hi_i = int(np.argmin(above)), int(np.argmax(above))
        ratio = lambda j: R.mp_of(got[2 + k][j]) / R.exp2_tab_exact_mp(sT[j], u[j], T)
        for j in list(np.argsort(above)[:16]) + list(np.argsort(above)[-16:]):
            assert 1 <= ratio(int(j)) <= top, (T, sT[j], u[j])
        print("[helper-probe] exp2_tab_above<%d> / exact: %.9f (sT = %r, u = %r) .. %.9f (sT = %r, u = %r); allowed 1 .. %.9f"
              % (T, float(above[lo_i]), sT[lo_i], u[lo_i], float(above[hi_i]), sT[hi_i], u[hi_i], top))
        assert above.min() >= 1 and above.max() <= top


@pytest.mark.parametrize("threads", [64, 128, 256])
def test_tables_on_the_device(dev, threads):
    """the two 2^(j/T) tables as staged in LDS, kAtanQ and the staged log10 table read back: every 2^(j/T) entry is the
    correctly rounded value, kAtanQ the once-rounded coefficients of its fit, the log10 table the header's [j][4] layout"""
    got = _f64(dev.run_n("TABLES", 512, threads))
    j = np.arange(512)
    _same_bits(_bits(got[0]), R.exp2_table(64)[j % 64], "2^(j/64) in LDS")
    _same_bits(_bits(got[1]), R.exp2_table(256)[j % 256], "2^(j/256) in LDS")
    _same_bits(_bits(got[2]), R.atan_q_fit()[j % 22], "kAtanQ")
    _same_bits(_bits(got[3]), R.log_table_words()[j % 128], "log10 table in LDS")


@pytest.mark.parametrize("threads", MATH_THREADS)
def test_exp2_dd(dev, threads):
    """exp2_dd(hi, lo) against 2^(hi + lo), |hi| < 1000, |lo| < 2^-40: hi - rint(hi) is exact; f = fl((hi - k) + lo) lies in
    [-1/2, 1/2] for these inputs and is off by at most half an ulp there, 2^-55, a factor 2^(2^-55) on the result; exp2_poly
    adds its 2e-16; ldexp is exact.  Bound: (1 + 2e-16) 2^(2^-55) - 1 = 2.193e-16."""
    hi, lo = R.exp2_dd_inputs()
    got = _f64(dev.run("EXP2_DD", [hi, lo], threads)[0])
    k = np.rint(hi)
    exact = np.ldexp(np.exp2((hi - k).astype(R.LD) + lo.astype(R.LD)), k.astype(np.int64))
    bound = float((1 + mpmath.mpf("2e-16")) * mpmath.power(2, mpmath.mpf(2) ** -55) - 1)
    err, i, gap = R.worst_case(R.rel_err_ld(got, exact), lambda j: mpmath.power(2, R.mp_of(hi[j]) + R.mp_of(lo[j])), got, "rel")
    _report("exp2_dd (relative)", err, "", bound, "hi = %r, lo = %r" % (hi[i], lo[i]))
    assert err <= bound and gap <= 2.0 ** -60


@pytest.mark.parametrize("threads", MATH_THREADS)
def test_dd_add(dev, threads):
    """dd_add against exact rational sums: hi + lo equals the exact sum of the four parts to 2^-100 -- the figure DESIGN.md
    uses for tail_sum -- relative to the sum for addends of one sign (what the prefix sums add, far apart included) and, for
    cancelling pairs, relative to the larger addend (the roundings are relative to the operands; a difference has no bound
    relative to itself); |lo| <= ulp(hi) / 2; a pair and its negative give exactly zero."""
    (h, l), (xh, xl), kinds = R.dd_inputs()
    got = _f64(dev.run("DD_ADD", [np.stack([h, l]), np.stack([xh, xl])], threads))
    exact = R.dd_exact(h, l, xh, xl)
    worst = {}
    for j, want in enumerate(exact):
        gh, gl = float(got[0][j]), float(got[1][j])
        scale = abs(want) if kinds[j] < 2 else max(abs(Fraction(float(h[j]))), abs(Fraction(float(xh[j]))))
        err = abs(Fraction(gh) + Fraction(gl) - want) / scale
        if err >= worst.get(kinds[j], (-1,))[0]:
            worst[kinds[j]] = (err, j)
        assert err <= Fraction(1, 2 ** 100), (j, gh, gl)
        assert abs(Fraction(gl)) <= Fraction(float(np.ldexp(0.5, int(np.frexp(gh)[1]) - 53))) if gh else gl == 0, (j, gh, gl)
    assert (got[0][kinds == 3] == 0).all() and (got[1][kinds == 3] == 0).all()
    for k, what in enumerate(("one sign", "far apart", "near negatives", "exact negatives", "partial cancellation")):
        err, j = worst[k]
        _report("dd_add, " + what, float(err), "= 2^%.1f" % (np.log2(float(err)) if err else -np.inf), 2.0 ** -100,
                "(%r, %r) + (%r, %r)" % (h[j], l[j], xh[j], xl[j]))


# ------------------------------------------------------------------------------------------------ atan, SPL
@pytest.mark.parametrize("threads", MATH_THREADS)
def test_atan_pos(dev, threads):
    """atan_pos on x >= 0 -- 0 (exactly 0), denormals, [0, 1], both sides of 1 to the last ulp, (1, 200] -- <= 2 ulp"""
    x = R.atan_inputs()
    got = _f64(dev.run("ATAN_POS", [x], threads)[0])
    assert got[0] == 0 and not np.signbit(got[0])
    pos = np.flatnonzero(x > 0)
    err, i, gap = R.worst_case(R.ulp_err_ld(got[pos], np.arctan(x[pos].astype(R.LD))), lambda j: mpmath.atan(R.mp_of(x[pos[j]])),
                               got[pos], "ulp")
    _report("atan_pos", err, "ulp", 2.0, "x = %r" % x[pos[i]])
    assert err <= 2.0 and gap <= 2.0 ** -9


@pytest.mark.parametrize("threads", MATH_THREADS)
def test_spl_db_tab_and_log10(dev, threads, tmp_path):
    """log10_tab32 as the device runs it, on the argument classes of tests/test_abi.py::test_table_log10_accuracy and to its
    bounds: <= 0.6 ulp where |log10 x| >= 1/4, <= 4e-17 absolute near 1; bit for bit the host build of the same header;
    spl_db_tab is fmax(96 + 10 log10_tab32, -30) of it, excess_plain the difference of two of those; the edges of spl_db_tab
    and of the plain spl_db: 0, denormals, negative values and NaN give -30.0, +inf stays +inf, the smallest normal is finite"""
    x = R.log10_inputs()
    a2 = x[::-1].copy()
    got = _f64(dev.run("SPL", [x, a2], threads))
    l10 = got[2]
    exact = np.log10(x.astype(R.LD))
    wide = np.abs(exact) >= 0.25
    iw, inr = np.flatnonzero(wide), np.flatnonzero(~wide)
    err, i, gap = R.worst_case(R.ulp_err_ld(l10[iw], exact[iw]), lambda j: mpmath.log10(R.mp_of(x[iw[j]])), l10[iw], "ulp")
    _report("log10_tab32, |log10 x| >= 1/4", err, "ulp", 0.6, "x = %r" % x[iw[i]])
    assert err <= 0.6 and gap <= 2.0 ** -9
    abs_ld = np.abs(l10[inr].astype(R.LD) - exact[inr])
    cand = inr[np.argsort(abs_ld)[-24:]]
    abs_mp = [abs(R.mp_of(l10[j]) - mpmath.log10(R.mp_of(x[j]))) for j in cand]
    k = int(np.argmax([float(e) for e in abs_mp]))
    _report("log10_tab32 near 1 (absolute)", float(abs_mp[k]), "", 4e-17, "x = %r" % x[cand[k]])
    assert abs_mp[k] <= 4e-17
    # the host build of the same header
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "log10_eval")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-I", os.path.join(root, "mrcaudiocodec_amd", "csrc"),
                           os.path.join(root, "tests", "log10_eval.cpp"), "-o", exe])
    host = np.frombuffer(subprocess.run([exe], input=x.tobytes(), stdout=subprocess.PIPE, check=True).stdout, dtype=np.float64)
    _same_bits(_bits(l10), host, "log10_tab32: device against the host build")
    # the wiring around it
    spl = np.maximum(96 + 10 * l10, -30.0)
    _same_bits(_bits(got[0]), spl, "spl_db_tab")
    assert (got[0] > -30).any() and (got[0] == -30).any()
    _same_bits(_bits(got[4]), spl, "excess_plain's threshold")
    _same_bits(_bits(got[3]), (spl[::-1] - 6.0 * 3) - spl, "excess_plain")
    plain = np.maximum(96 + 10 * exact, -30.0)
    # the plain spl_db: the library's log10 (3 ulp of at most 308, OpenCL's requirement: 1.7e-13), times 10, two roundings of
    # at most half an ulp of 4096 each
    assert np.abs(got[1].astype(R.LD) - plain).max() <= 10 * 3 * 2.0 ** -44 + 2.0 ** -41
    # edges
    e = R.SPL_EDGES
    ge = _f64(dev.run("SPL", [e, np.ones(len(e))], threads))
    for k, what in ((0, "spl_db_tab"), (1, "spl_db")):
        for v, r in zip(e, ge[k]):
            if v == np.inf:
                assert r == np.inf, (what, v, r)
            else:
                assert r == -30.0 and np.isfinite(r), (what, v, r)
    tiny = np.finfo(float).tiny
    gt = _f64(dev.run("SPL", [np.array([tiny]), np.ones(1)], threads))
    assert np.isfinite(gt[2][0]) and R.ulp_err_mp(gt[2][0], mpmath.log10(R.mp_of(tiny))) <= 0.6


# ------------------------------------------------------------------------------------------------ quantiser
@pytest.mark.parametrize("threads", [64, 256])
def test_mag_code_unsigned_against_long_long_and_exact(dev, threads):
    """mag_code<unsigned> (the encoder's) against mag_code<long long> (the L1 entry points') and the exact restatement of
    quantize.py:12-38, every nBits 2..31: the rational rounding edges of ((2^nBits - 1) mag + 1) / 2 with the doubles either
    side, the smallest magnitude with a non-zero code, 0, the double below 1.0 and 1.0"""
    mags, bits = R.mag_code_inputs()
    got = _i64(dev.run("MAG_CODE", [mags, bits], threads))
    want = np.array([R.mag_code_exact(float(m), int(b)) for m, b in zip(mags, bits)], dtype=np.int64)
    assert np.array_equal(got[0], got[1])
    bad = np.flatnonzero(got[0] != want)
    assert bad.size == 0, (mags[bad[0]], bits[bad[0]], got[0][bad[0]], want[bad[0]])
    assert len(set(want.tolist())) > 200 and (want == 0).any()


@pytest.mark.parametrize("threads", [64, 256])
def test_scale_factor_and_mantissa_unsigned(dev, threads):
    """scale_factor_dev and mantissa_dev with Code = unsigned against Code = long long and the exact restatement of
    quantize.py:114-146, 294-322: every scale 0 .. cap for nScaleBits 1..4 and nMantBits 2..16, both signs, at the code
    width's edge magnitudes"""
    x, sc, sb, mb = R.scale_mant_inputs()
    got = _i64(dev.run("SCALE_MANT", [x, sc | (sb << 8) | (mb << 16)], threads))
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[2], got[3])
    sf = np.array([R.scale_factor_exact(float(v), int(s), int(m)) for v, s, m in zip(x, sb, mb)])
    mant = np.array([R.mantissa_exact(float(v), int(k), int(s), int(m)) for v, k, s, m in zip(x, sc, sb, mb)])
    bad = np.flatnonzero(got[0] != sf)
    assert bad.size == 0, (x[bad[0]], sb[bad[0]], mb[bad[0]], got[0][bad[0]], sf[bad[0]])
    bad = np.flatnonzero(got[2] != mant)
    assert bad.size == 0, (x[bad[0]], sc[bad[0]], sb[bad[0]], mb[bad[0]], got[2][bad[0]], mant[bad[0]])
    neg = x < 0
    assert (got[2][neg] >= (1 << (mb[neg] - 1))).all() and len(set(sf.tolist())) == 16
