// fp64 and wavefront helpers of the masking kernels (mrc_kernels_smr*.hip): order-preserving keys, 2^x by polynomial and by
// table, double-double sums, wave-wide sums of blocks of values in registers, 1/x, atan, and the table-driven SPL conversion
// with the two device tables every masking kernel stages (2^(j/64), log10).
#pragma once
#include "mrc_device.hpp"

#include "mrc_log10.hpp"

namespace mrc {
using namespace dev;
namespace {

// Order-preserving map double -> uint64 (a < b  <=>  key(a) < key(b), -0 < +0), so that a maximum over
// doubles can be taken with an integer LDS atomic.
__device__ __forceinline__ unsigned long long order_key(double v) {
    unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double order_value(unsigned long long k) {
    unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

constexpr double kLog2Of10 = 0x1.a934f0979a371p+1;     // log2(10) = hi + lo
constexpr double kLog2Of10Lo = 0x1.7f2495fb7fa6dp-53;
// b = -2.7*log2(10) bits per Bark below the masker (psychoac.py:74), split hi + lo
constexpr double kLowHi = -0x1.1f03bbffee7edp+3;
constexpr double kLowLo = 0x1.e3c74df63d090p-51;

// 2^f on [-0.5, 0.5]: degree-11 Chebyshev-node fit, max relative error 2e-16 including evaluation.
__device__ __forceinline__ double exp2_poly(double f) {
    double p = 0x1.e9ec1fcb69a7fp-32;
    p = fma(p, f, 0x1.e6228acd1c6e5p-28);
    p = fma(p, f, 0x1.b524ebd13a55fp-24);
    p = fma(p, f, 0x1.62bfc2c86d700p-20);
    p = fma(p, f, 0x1.ffcbfc6da6ed1p-17);
    p = fma(p, f, 0x1.430913112c61bp-13);
    p = fma(p, f, 0x1.5d87fe78a3f9cp-10);
    p = fma(p, f, 0x1.3b2ab6fb9f1a5p-7);
    p = fma(p, f, 0x1.c6b08d704a0c6p-5);
    p = fma(p, f, 0x1.ebfbdff82c5aep-3);
    p = fma(p, f, 0x1.62e42fefa39efp-1);
    return fma(p, f, 1.0);
}

// 2^(sT*u/T) for the spreading loop, table driven (T = kExpTab entries per octave, sT = slope in 1/T bit per Bark):
// n = rint(sT*u) splits into k = n / T (exponent), j = n mod T (entry of the 2^(j/T) table in LDS) and a remainder
// g = sT*u - n in [-1/2, 1/2] (one rounding, by fma) whose 2^(g/T) = exp(g ln2/T) is a Taylor polynomial (T = 64: degree 5,
// remainder |x|^6/6! e^|x| < 3.53e-17 of the value at |x| <= ln2/128).  With the correctly rounded table entry, the last fma
// of the chain and the product, one rounding each, the result is within 3.70e-16 (T = 256: 3.73e-16) of 2^(sT*u/T); derived
// and held on the device by tests/test_gpu_helper_probes.py.  sT*u == 0 gives exactly 1 (a line inside +-1/2 Bark
// gets exactly the masker's intensity).  Requires |sT*u| < 2^31 (here it is < 16000).
constexpr int kExpTab = 64;
constexpr int kExpTabShift = 6;
// an SPL reaches its -30 dB floor at an intensity of 10^-12.6 (psychoac.py:8-12); above this guard it does not
constexpr double kSplFloorGuard = 1e-12;
// T = 256 (kExpTabLong, the long block's sweep): a table four times as fine takes one term off the polynomial
// (|x ln2 / 256|^5 / 5! < 4e-17 for the remainder |x| <= 1/2); smr_kernel 4.499 against 4.546 ms with T = 64.
constexpr int kExpTabLong = 256;
template <int T = kExpTab>
__device__ __forceinline__ double exp2_tab64(double sT, double u, const double* __restrict__ tab) {
    const double shifter = 0x1.8p52;
    const double tt = fma(sT, u, shifter);
    const double r = tt - shifter;
    const double g = fma(sT, u, -r);
    const int n = __double2loint(tt);
    if (T == 256) {
        double p = fma(0x1.3b2ab6fba4e77p-39, g, 0x1.c6b08d704a0c0p-29);
        p = fma(p, g, 0x1.ebfbdff82c58fp-19);
        p = fma(p, g, 0x1.62e42fefa39efp-9);
        p = fma(p, g, 1.0);
        return ldexp(p * tab[n & 255], n >> 8);
    }
    double p = fma(0x1.5d87fe78a6731p-40, g, 0x1.3b2ab6fba4e77p-31);
    p = fma(p, g, 0x1.c6b08d704a0c0p-23);
    p = fma(p, g, 0x1.ebfbdff82c58fp-15);
    p = fma(p, g, 0x1.62e42fefa39efp-7);
    p = fma(p, g, 1.0);
    // (the table as two arrays of 32-bit halves -- entry j of either in bank j, conflict-free for any index pattern -- was
    // measured in round 3: 4.60 against 4.54 ms; like the 32-entry table of round 2 it removes conflicts the waves do not wait for)
    return ldexp(p * tab[n & (kExpTab - 1)], n >> kExpTabShift);
}

// An UPPER BOUND of the same 2^(sT*u/T) from the table alone: with n = rint(sT*u), sT*u <= n + 1/2 < n + 1, so entry n + 1
// (correctly rounded: within 2^-53 of 2^((n+1)/T)) is above it, by at most 2^(3/(2T)) - 1 (T = 256: 0.41 %).  No polynomial.
template <int T>
__device__ __forceinline__ double exp2_tab_above(double sT, double u, const double* __restrict__ tab) {
    static_assert(T == kExpTab || T == kExpTabLong, "the tables staged in LDS");
    const int n = __double2loint(fma(sT, u, 0x1.8p52)) + 1;
    return ldexp(tab[n & (T - 1)], n >> (T == kExpTabLong ? 8 : kExpTabShift));
}

// 2^(j/64), j = 0..63, correctly rounded
__constant__ double kExp2Tab[kExpTab] = {
    0x1.0000000000000p+0, 0x1.02c9a3e778061p+0, 0x1.059b0d3158574p+0, 0x1.0874518759bc8p+0,
    0x1.0b5586cf9890fp+0, 0x1.0e3ec32d3d1a2p+0, 0x1.11301d0125b51p+0, 0x1.1429aaea92de0p+0,
    0x1.172b83c7d517bp+0, 0x1.1a35beb6fcb75p+0, 0x1.1d4873168b9aap+0, 0x1.2063b88628cd6p+0,
    0x1.2387a6e756238p+0, 0x1.26b4565e27cddp+0, 0x1.29e9df51fdee1p+0, 0x1.2d285a6e4030bp+0,
    0x1.306fe0a31b715p+0, 0x1.33c08b26416ffp+0, 0x1.371a7373aa9cbp+0, 0x1.3a7db34e59ff7p+0,
    0x1.3dea64c123422p+0, 0x1.4160a21f72e2ap+0, 0x1.44e086061892dp+0, 0x1.486a2b5c13cd0p+0,
    0x1.4bfdad5362a27p+0, 0x1.4f9b2769d2ca7p+0, 0x1.5342b569d4f82p+0, 0x1.56f4736b527dap+0,
    0x1.5ab07dd485429p+0, 0x1.5e76f15ad2148p+0, 0x1.6247eb03a5585p+0, 0x1.6623882552225p+0,
    0x1.6a09e667f3bcdp+0, 0x1.6dfb23c651a2fp+0, 0x1.71f75e8ec5f74p+0, 0x1.75feb564267c9p+0,
    0x1.7a11473eb0187p+0, 0x1.7e2f336cf4e62p+0, 0x1.82589994cce13p+0, 0x1.868d99b4492edp+0,
    0x1.8ace5422aa0dbp+0, 0x1.8f1ae99157736p+0, 0x1.93737b0cdc5e5p+0, 0x1.97d829fde4e50p+0,
    0x1.9c49182a3f090p+0, 0x1.a0c667b5de565p+0, 0x1.a5503b23e255dp+0, 0x1.a9e6b5579fdbfp+0,
    0x1.ae89f995ad3adp+0, 0x1.b33a2b84f15fbp+0, 0x1.b7f76f2fb5e47p+0, 0x1.bcc1e904bc1d2p+0,
    0x1.c199bdd85529cp+0, 0x1.c67f12e57d14bp+0, 0x1.cb720dcef9069p+0, 0x1.d072d4a07897cp+0,
    0x1.d5818dcfba487p+0, 0x1.da9e603db3285p+0, 0x1.dfc97337b9b5fp+0, 0x1.e502ee78b3ff6p+0,
    0x1.ea4afa2a490dap+0, 0x1.efa1bee615a27p+0, 0x1.f50765b6e4540p+0, 0x1.fa7c1819e90d8p+0
};

// 2^(hi + lo), |lo| << 1
__device__ __forceinline__ double exp2_dd(double hi, double lo) {
    const double k = rint(hi);
    return ldexp(exp2_poly((hi - k) + lo), (int)k);
}

// (hi, lo) += (xh, xl) in double-double (Knuth two-sum on the high parts; |lo| << |hi|)
__device__ __forceinline__ void dd_add(double* hi, double* lo, double xh, double xl) {
    const double s = *hi + xh;
    const double v = s - *hi;
    double e = (*hi - (s - v)) + (xh - v);
    e += *lo + xl;
    const double h = s + e;
    *lo = e - (h - s);
    *hi = h;
}

// Cross-lane primitives of the coefficient reduction, all register-to-register (no LDS round trips):
//   distance 32 / 16: gfx950's v_permlane32_swap / v_permlane16_swap exchange the upper half (odd 16-lane rows) of one
//                     register with the lower half (even rows) of another -- exactly one step of a transposing
//                     butterfly: afterwards the lower lanes hold both halves' `a`, the upper lanes both halves' `b`;
//   distance 8, 4, 2, 1: DPP row rotate / half mirror / quad permutes.
template <int DIST>
__device__ __forceinline__ double wave_xchg_add(double a, double b) {
    double x, y;
    rows_swap<DIST>(a, b, &x, &y);
    return x + y;
}
// Sum each of 8 per-lane values over the 64 lanes of the wave and leave the 8 totals in every lane (wave-uniform).
// Transposing butterfly: at distances 32, 16, 8 a lane hands HALF of its remaining values to its partner and adds
// the partner's half of the others (4 + 2 + 1 exchanges instead of 8 x 6); three plain steps finish the one value
// left per lane; the lane group [8j, 8j+8) then holds the total of value j.
template <int W>
__device__ __forceinline__ void wave_sum_block(double* v, int lane) {
    static_assert(W == 8, "block of 8 values");
    const double a0 = wave_xchg_add<32>(v[0], v[4]);           // lanes 0..31 keep values 0..3, lanes 32..63 values 4..7
    const double a1 = wave_xchg_add<32>(v[1], v[5]);
    const double a2 = wave_xchg_add<32>(v[2], v[6]);
    const double a3 = wave_xchg_add<32>(v[3], v[7]);
    const double b0 = wave_xchg_add<16>(a0, a2);               // even rows keep the lower pair, odd rows the upper
    const double b1 = wave_xchg_add<16>(a1, a3);
    const double s0 = b0 + dpp_move<0x128>(b0);                // row_ror:8 = lane ^ 8
    const double s1 = b1 + dpp_move<0x128>(b1);
    double s = (lane & 8) ? s1 : s0;
    s += dpp_move<0xB1>(s);                                    // quad_perm [1,0,3,2]
    s += dpp_move<0x4E>(s);                                    // quad_perm [2,3,0,1]
    s += dpp_move<0x141>(s);                                   // row_half_mirror: the other quad of the 8-lane group
#pragma unroll
    for (int j = 0; j < W; ++j)
        v[j] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(s), j * (kWave / W)),
                                __builtin_amdgcn_readlane(__double2loint(s), j * (kWave / W)));
}

// Sum each of N per-lane values over the 64 lanes and leave all N totals in every lane: blocks of 8 (a block of 16 would save
// three exchanges per 16 values but keeps 24 doubles live at once), values beyond the last full block one by one
template <int N>
__device__ __forceinline__ void wave_sum_all(double* v, int lane) {
    constexpr int n8 = N / 8;
#pragma unroll
    for (int i = 0; i < n8; ++i) wave_sum_block<8>(v + 8 * i, lane);
#pragma unroll
    for (int j = 8 * n8; j < N; ++j) {
        v[j] = wave_sum(v[j]);
    }
}

// 1/x for a finite positive normal x: hardware estimate + two Newton steps (relative error ~2^-52; NOT the correctly
// rounded quotient -- used by the fast spreading mode only, where one more rounding per masker / line is inside what the
// FFT in front of it already differs from the reference's by; the EXACT mode divides like the reference).  The 2^-52 is for
// x <= 2^1022: beyond it 1/x is subnormal, on a grid of 2^-1074 that no result can beat, and the last step's rounding leaves
// the result within 1.5 x 2^-1074 of 1/x.  The thresholds it divides by end far below that or at +inf (line_ratio).
__device__ __forceinline__ double recip_nr(double x) {
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    return fma(fma(-x, r, 1.0), r, r);
}
// The ratio form of the band maximum (a2 / t) and a threshold of +inf: from ~80 kHz on, Intensity(Thresh(f)) of the top lines
// overflows (psychoac.py:14-25), and recip_nr(+inf) is NaN (rcp gives 0, then -inf * 0).  As an atomicMax key a NaN beats every
// ratio of the band and then drops out of the band's fmax, leaving the band at -1e300.  The line's true ratio is 0 (an excess of
// -inf, never the band's maximum: a band's lower lines have finite thresholds), and fmax(q, 0) gives exactly that -- q >= 0
// otherwise, and one v_max per line is all it costs.
__device__ __forceinline__ double line_ratio(double a2, double t) { return fmax(a2 * recip_nr(t), 0.0); }
// atan(x) for x >= 0 (psychoac.py:27-29's two calls per masker), <= 2 ulp: x <= 1: x Q(x^2), Q of degree 21 from a
// Chebyshev fit in 60-digit arithmetic (tools/make_atan_poly.py); x > 1: pi/2 - atan(1/x).  ~40 instructions against the
// ~90 of the library's.
__device__ constexpr double kAtanQ[22] = {0x1.0000000000000p+0, -0x1.5555555555546p-2, 0x1.999999999861ep-3, -0x1.2492492443a94p-3, 0x1.c71c71b1fed92p-4, -0x1.745d1586bfed2p-4, 0x1.3b1398601e89dp-4, -0x1.1110151cb4f09p-4, 0x1.e1d315290f292p-5, -0x1.aed3667a4693ap-5, 0x1.849ab97c0d9e6p-5, -0x1.5eda2e1403e06p-5, 0x1.385c01bcb507ap-5, -0x1.0b657ae92d3e9p-5, 0x1.a91e0c9b2881ep-6, -0x1.2d3ffbb3d4964p-6, 0x1.6c7238a2d8193p-7, -0x1.6773524f49226p-8, 0x1.12060552e1b82p-9, -0x1.2c4eeb1fa7a5bp-11, 0x1.a2865ec94274cp-14, -0x1.156d8b1441eeep-17};
__device__ __forceinline__ double atan_pos(double x) {
    const bool big = x > 1.0;
    const double t = big ? recip_nr(x) : x;
    const double u = t * t;
    double q = kAtanQ[21];
#pragma unroll
    for (int i = 20; i >= 0; --i) q = fma(q, u, kAtanQ[i]);
    const double a = t * q;
    return big ? (0x1.921fb54442d18p+0 - a) + 0x1.1a62633145c07p-54 : a;
}

// kLog10Tab as [j][4] for the LDS copy
struct LogTabDev { double v[kLogTabEntries * 4]; };
constexpr LogTabDev make_log_tab() {
    LogTabDev t{};
    for (int j = 0; j < kLogTabEntries; ++j)
        for (int c = 0; c < 3; ++c) t.v[4 * j + c] = kLog10Tab[j][c];
    return t;
}
__constant__ LogTabDev kLogTabDev = make_log_tab();

// psychoac.py:8-12 with the table-driven log10 (mrc_log10.hpp).  Anything below the smallest normal number -- zero,
// denormals, negative values -- is more than 3000 dB under the -30 dB floor (a NaN ends there too, as with fmax in
// spl_db); +inf stays +inf.
__device__ __forceinline__ double spl_db_tab(double intensity, const double* __restrict__ tab) {
    if (!(intensity >= 0x1p-1022)) return -30.0;
    if (intensity > 0x1.fffffffffffffp+1023) return intensity;
    return fmax(96 + 10 * log10_tab32(intensity, tab), -30.0);
}

// The reference's own per-line formula (psychoac.py:173,212), for lines whose SPL sits on the -30 dB floor and for
// callers that want the thresholds.  Rare on the full path and deliberately OUT OF LINE: inlined, its constants would
// be hoisted out of the sweep loop and cost registers (and scratch traffic) in every frame.
__device__ __attribute__((noinline)) double excess_plain(double t, double a2, int scale, const double* tab, double* thrOut) {
    const double thr = spl_db_tab(t, tab);
    *thrOut = thr;
    return (spl_db_tab(a2, tab) - 6. * scale) - thr;
}

}  // namespace
}  // namespace mrc
