// What smr_body (mrc_smr_body.hpp) is made of, for the units that compile smr_kernel: the layout of its dynamic LDS, the
// far and near field of the sorted sweep, the slope nodes, and the 2^(j/256) table of the long block's sweep.
#pragma once
#include "mrc_smr_math.hpp"
#include "mrc_smr_profile.hpp"

namespace mrc {
using namespace dev;
namespace {

// Where the staged tables sit in the dynamic LDS (offsets in doubles, chosen by launch_smr): the Bark grid of the
// lines for the masker-side searches, the log10 table, the first quadrant of the FFT twiddles (-1: use global).
struct SmrLds { int zbOff, logOff, twOff; };
// The layout for a block of H FFT points, M lines and `last` searched bins; *total = doubles of dynamic LDS.  One function
// for the launcher (any shape) and, evaluated at compile time, for the kernels specialised on the block dimensions.
__host__ __device__ constexpr SmrLds smr_layout(int H, int M, int last, int* totalOut) {
    int total = 4 * H + last + 1;
    const int pkShorts = (last / 2 + 5) & ~3;
    const int piOff = 2 * H + (pkShorts * 2 + 2 * (M + 2) * 2) / 8;          // where piHi starts (kernel layout)
    const int piLen = 2 * (last / 2 + 2);
    const int logLen = kLogTabEntries * 4;
    SmrLds lay{0, 0, -1};
    if (piOff + (piLen > M ? piLen : M) + logLen <= 4 * H) {
        lay.zbOff = piOff;                               // overwritten by the prefix sums after the searches
        lay.logOff = 4 * H - logLen;
    } else {
        total += total & 1;
        lay.zbOff = total;
        lay.logOff = total + M;
        total += M + logLen;
    }
    if ((H & (H - 1)) == 0 && H >= 16) {                 // first quadrant of the FFT twiddles: in the spectrum area
        if (H / 2 <= last + 1) lay.twOff = 4 * H;
        else { total += total & 1; lay.twOff = total; total += H / 2; }
    }
    if (totalOut) *totalOut = total;
    return lay;
}

// The suffix scans over a frame's maskers (smr_body) hold kWave * kSmrMaxSeg entries: at most that many peaks + 1 per block,
// which bounds the block sizes the kernel takes (smr_peaks_fit)
constexpr int kSmrMaxSeg = 8;

// Slope nodes: the most maskers a block of DIM lines can take through them.  Rows of kNodeCols doubles for every fourth
// masker (+ row 0) lie between the per-line counts and the log10 table (where the peak bins and the Bark grid were); the masker
// table (4 P) and the in-band prefix sums (2 (P + 1)) share the first FFT buffer with the band keys and the 2^x table (96).
__host__ __device__ constexpr int node_max_maskers(int DIM) {
    const SmrLds lay = smr_layout(DIM, DIM, DIM - 100, nullptr);
    const int qStart = 2 * DIM + (2 * (DIM + 2) * 2) / 8;               // behind cnt / nUp ((DIM + 2) uint16 each)
    if (lay.logOff <= qStart || lay.logOff >= 4 * DIM) return 0;        // (the log10 table is not behind the rows in this layout)
    const int rows = (lay.logOff - qStart) / 18;
    const int byRows = (rows - 1) * 4, byTable = (2 * DIM - 96 - 2) / 6, bySeg = 3 * 26 * 4 - 4;
    int m = byRows < byTable ? byRows : byTable;
    m = m < bySeg ? m : bySeg;
    return m < 0 ? 0 : m;
}
static_assert(node_max_maskers(1024) == 308, "long block: 78 rows");

// far-field expansion (see the sweep): highest order, fewest maskers worth it, and for each supported order J the
// largest |x| with |x|^(J+1)/(J+1)! e^|x| below 1e-15 (x = slope spread * half the Bark span of a group of lines)
// Orders 8 / 12 / 16: order 20 (limit 1.3) costs 48 accumulator registers and spilled around every chunk.  The limits keep the
// truncated tail below 1e-15 of each term: 2 % faster than the first version's 1e-17 (0.052 / 0.27 / 0.68; more chunks get by
// with a lower order, the thresholds move < 1e-14 dB); 1e-13 (0.1466 / 0.5436 / 1.1529) gained another 1.2 % and was not taken.
constexpr int kFarMaxOrder = 16;
constexpr int kFarMinMaskers = 24;
constexpr double kFarLimit8 = 0.089, kFarLimit12 = 0.397, kFarLimit16 = 0.94;
constexpr double kInvFactorial[kFarMaxOrder + 1] = {
    1.0, 1.0, 1.0 / 2, 1.0 / 6, 1.0 / 24, 1.0 / 120, 1.0 / 720, 1.0 / 5040, 1.0 / 40320, 1.0 / 362880,
    1.0 / 3628800, 1.0 / 39916800, 1.0 / 479001600, 1.0 / 6227020800.0, 1.0 / 87178291200.0,
    1.0 / 1307674368000.0, 1.0 / 20922789888000.0};

// 2^(j/256), j = 0..255, correctly rounded (the long block's table)
__constant__ double kExp2Tab256[256] = {
    0x1.0000000000000p+0, 0x1.00b1afa5abcbfp+0, 0x1.0163da9fb3335p+0, 0x1.02168143b0281p+0,
    0x1.02c9a3e778061p+0, 0x1.037d42e11bbccp+0, 0x1.04315e86e7f85p+0, 0x1.04e5f72f654b1p+0,
    0x1.059b0d3158574p+0, 0x1.0650a0e3c1f89p+0, 0x1.0706b29ddf6dep+0, 0x1.07bd42b72a836p+0,
    0x1.0874518759bc8p+0, 0x1.092bdf66607e0p+0, 0x1.09e3ecac6f383p+0, 0x1.0a9c79b1f3919p+0,
    0x1.0b5586cf9890fp+0, 0x1.0c0f145e46c85p+0, 0x1.0cc922b7247f7p+0, 0x1.0d83b23395decp+0,
    0x1.0e3ec32d3d1a2p+0, 0x1.0efa55fdfa9c5p+0, 0x1.0fb66affed31bp+0, 0x1.1073028d7233ep+0,
    0x1.11301d0125b51p+0, 0x1.11edbab5e2ab6p+0, 0x1.12abdc06c31ccp+0, 0x1.136a814f204abp+0,
    0x1.1429aaea92de0p+0, 0x1.14e95934f312ep+0, 0x1.15a98c8a58e51p+0, 0x1.166a45471c3c2p+0,
    0x1.172b83c7d517bp+0, 0x1.17ed48695bbc0p+0, 0x1.18af9388c8deap+0, 0x1.1972658375d2fp+0,
    0x1.1a35beb6fcb75p+0, 0x1.1af99f8138a1cp+0, 0x1.1bbe084045cd4p+0, 0x1.1c82f95281c6bp+0,
    0x1.1d4873168b9aap+0, 0x1.1e0e75eb44027p+0, 0x1.1ed5022fcd91dp+0, 0x1.1f9c18438ce4dp+0,
    0x1.2063b88628cd6p+0, 0x1.212be3578a819p+0, 0x1.21f49917ddc96p+0, 0x1.22bdda27912d1p+0,
    0x1.2387a6e756238p+0, 0x1.2451ffb82140ap+0, 0x1.251ce4fb2a63fp+0, 0x1.25e85711ece75p+0,
    0x1.26b4565e27cddp+0, 0x1.2780e341ddf29p+0, 0x1.284dfe1f56381p+0, 0x1.291ba7591bb70p+0,
    0x1.29e9df51fdee1p+0, 0x1.2ab8a66d10f13p+0, 0x1.2b87fd0dad990p+0, 0x1.2c57e39771b2fp+0,
    0x1.2d285a6e4030bp+0, 0x1.2df961f641589p+0, 0x1.2ecafa93e2f56p+0, 0x1.2f9d24abd886bp+0,
    0x1.306fe0a31b715p+0, 0x1.31432edeeb2fdp+0, 0x1.32170fc4cd831p+0, 0x1.32eb83ba8ea32p+0,
    0x1.33c08b26416ffp+0, 0x1.3496266e3fa2dp+0, 0x1.356c55f929ff1p+0, 0x1.36431a2de883bp+0,
    0x1.371a7373aa9cbp+0, 0x1.37f26231e754ap+0, 0x1.38cae6d05d866p+0, 0x1.39a401b7140efp+0,
    0x1.3a7db34e59ff7p+0, 0x1.3b57fbfec6cf4p+0, 0x1.3c32dc313a8e5p+0, 0x1.3d0e544ede173p+0,
    0x1.3dea64c123422p+0, 0x1.3ec70df1c5175p+0, 0x1.3fa4504ac801cp+0, 0x1.40822c367a024p+0,
    0x1.4160a21f72e2ap+0, 0x1.423fb2709468ap+0, 0x1.431f5d950a897p+0, 0x1.43ffa3f84b9d4p+0,
    0x1.44e086061892dp+0, 0x1.45c2042a7d232p+0, 0x1.46a41ed1d0057p+0, 0x1.4786d668b3237p+0,
    0x1.486a2b5c13cd0p+0, 0x1.494e1e192aed2p+0, 0x1.4a32af0d7d3dep+0, 0x1.4b17dea6db7d7p+0,
    0x1.4bfdad5362a27p+0, 0x1.4ce41b817c114p+0, 0x1.4dcb299fddd0dp+0, 0x1.4eb2d81d8abffp+0,
    0x1.4f9b2769d2ca7p+0, 0x1.508417f4531eep+0, 0x1.516daa2cf6642p+0, 0x1.5257de83f4eefp+0,
    0x1.5342b569d4f82p+0, 0x1.542e2f4f6ad27p+0, 0x1.551a4ca5d920fp+0, 0x1.56070dde910d2p+0,
    0x1.56f4736b527dap+0, 0x1.57e27dbe2c4cfp+0, 0x1.58d12d497c7fdp+0, 0x1.59c0827ff07ccp+0,
    0x1.5ab07dd485429p+0, 0x1.5ba11fba87a03p+0, 0x1.5c9268a5946b7p+0, 0x1.5d84590998b93p+0,
    0x1.5e76f15ad2148p+0, 0x1.5f6a320dceb71p+0, 0x1.605e1b976dc09p+0, 0x1.6152ae6cdf6f4p+0,
    0x1.6247eb03a5585p+0, 0x1.633dd1d1929fdp+0, 0x1.6434634ccc320p+0, 0x1.652b9febc8fb7p+0,
    0x1.6623882552225p+0, 0x1.671c1c70833f6p+0, 0x1.68155d44ca973p+0, 0x1.690f4b19e9538p+0,
    0x1.6a09e667f3bcdp+0, 0x1.6b052fa75173ep+0, 0x1.6c012750bdabfp+0, 0x1.6cfdcddd47645p+0,
    0x1.6dfb23c651a2fp+0, 0x1.6ef9298593ae5p+0, 0x1.6ff7df9519484p+0, 0x1.70f7466f42e87p+0,
    0x1.71f75e8ec5f74p+0, 0x1.72f8286ead08ap+0, 0x1.73f9a48a58174p+0, 0x1.74fbd35d7cbfdp+0,
    0x1.75feb564267c9p+0, 0x1.77024b1ab6e09p+0, 0x1.780694fde5d3fp+0, 0x1.790b938ac1cf6p+0,
    0x1.7a11473eb0187p+0, 0x1.7b17b0976cfdbp+0, 0x1.7c1ed0130c132p+0, 0x1.7d26a62ff86f0p+0,
    0x1.7e2f336cf4e62p+0, 0x1.7f3878491c491p+0, 0x1.80427543e1a12p+0, 0x1.814d2add106d9p+0,
    0x1.82589994cce13p+0, 0x1.8364c1eb941f7p+0, 0x1.8471a4623c7adp+0, 0x1.857f4179f5b21p+0,
    0x1.868d99b4492edp+0, 0x1.879cad931a436p+0, 0x1.88ac7d98a6699p+0, 0x1.89bd0a478580fp+0,
    0x1.8ace5422aa0dbp+0, 0x1.8be05bad61778p+0, 0x1.8cf3216b5448cp+0, 0x1.8e06a5e0866d9p+0,
    0x1.8f1ae99157736p+0, 0x1.902fed0282c8ap+0, 0x1.9145b0b91ffc6p+0, 0x1.925c353aa2fe2p+0,
    0x1.93737b0cdc5e5p+0, 0x1.948b82b5f98e5p+0, 0x1.95a44cbc8520fp+0, 0x1.96bdd9a7670b3p+0,
    0x1.97d829fde4e50p+0, 0x1.98f33e47a22a2p+0, 0x1.9a0f170ca07bap+0, 0x1.9b2bb4d53fe0dp+0,
    0x1.9c49182a3f090p+0, 0x1.9d674194bb8d5p+0, 0x1.9e86319e32323p+0, 0x1.9fa5e8d07f29ep+0,
    0x1.a0c667b5de565p+0, 0x1.a1e7aed8eb8bbp+0, 0x1.a309bec4a2d33p+0, 0x1.a42c980460ad8p+0,
    0x1.a5503b23e255dp+0, 0x1.a674a8af46052p+0, 0x1.a799e1330b358p+0, 0x1.a8bfe53c12e59p+0,
    0x1.a9e6b5579fdbfp+0, 0x1.ab0e521356ebap+0, 0x1.ac36bbfd3f37ap+0, 0x1.ad5ff3a3c2774p+0,
    0x1.ae89f995ad3adp+0, 0x1.afb4ce622f2ffp+0, 0x1.b0e07298db666p+0, 0x1.b20ce6c9a8952p+0,
    0x1.b33a2b84f15fbp+0, 0x1.b468415b749b1p+0, 0x1.b59728de5593ap+0, 0x1.b6c6e29f1c52ap+0,
    0x1.b7f76f2fb5e47p+0, 0x1.b928cf22749e4p+0, 0x1.ba5b030a1064ap+0, 0x1.bb8e0b79a6f1fp+0,
    0x1.bcc1e904bc1d2p+0, 0x1.bdf69c3f3a207p+0, 0x1.bf2c25bd71e09p+0, 0x1.c06286141b33dp+0,
    0x1.c199bdd85529cp+0, 0x1.c2d1cd9fa652cp+0, 0x1.c40ab5fffd07ap+0, 0x1.c544778fafb22p+0,
    0x1.c67f12e57d14bp+0, 0x1.c7ba88988c933p+0, 0x1.c8f6d9406e7b5p+0, 0x1.ca3405751c4dbp+0,
    0x1.cb720dcef9069p+0, 0x1.ccb0f2e6d1675p+0, 0x1.cdf0b555dc3fap+0, 0x1.cf3155b5bab74p+0,
    0x1.d072d4a07897cp+0, 0x1.d1b532b08c968p+0, 0x1.d2f87080d89f2p+0, 0x1.d43c8eacaa1d6p+0,
    0x1.d5818dcfba487p+0, 0x1.d6c76e862e6d3p+0, 0x1.d80e316c98398p+0, 0x1.d955d71ff6075p+0,
    0x1.da9e603db3285p+0, 0x1.dbe7cd63a8315p+0, 0x1.dd321f301b460p+0, 0x1.de7d5641c0658p+0,
    0x1.dfc97337b9b5fp+0, 0x1.e11676b197d17p+0, 0x1.e264614f5a129p+0, 0x1.e3b333b16ee12p+0,
    0x1.e502ee78b3ff6p+0, 0x1.e653924676d76p+0, 0x1.e7a51fbc74c83p+0, 0x1.e8f7977cdb740p+0,
    0x1.ea4afa2a490dap+0, 0x1.eb9f4867cca6ep+0, 0x1.ecf482d8e67f1p+0, 0x1.ee4aaa2188510p+0,
    0x1.efa1bee615a27p+0, 0x1.f0f9c1cb6412ap+0, 0x1.f252b376bba97p+0, 0x1.f3ac948dd7274p+0,
    0x1.f50765b6e4540p+0, 0x1.f6632798844f8p+0, 0x1.f7bfdad9cbe14p+0, 0x1.f91d802243c89p+0,
    0x1.fa7c1819e90d8p+0, 0x1.fbdba3692d514p+0, 0x1.fd3c22b8f71f1p+0, 0x1.fe9d96b2a23d9p+0
};

// Far field of one group of lines (see the sweep): maskers [0, nFar) lie more than 1/2 Bark below every line of
// the group.  With c the group's centre, d = z - c, a_m = s_m ln2 the masker's slope and A any reference slope,
//   sum_m I_m 2^(s_m (z - z_m - 1/2)) = exp(A d) sum_m e_m exp((a_m - A) d) = exp(A d) sum_j d^j/j! B_j,
//   e_m = I_m 2^(s_m (c - z_m - 1/2)),  B_j = sum_m e_m (a_m - A)^j.
// Lanes take maskers (ONE 2^x per masker and group instead of one per masker and line), the J+1 coefficients are
// wave-reduced, every line evaluates the polynomial and one 2^x.  The caller picks J from |a_m - A| |d|.
// NB = J + 1 padded to what wave_sum_all reduces cheapest.
template <int J, int NB, int T>
__device__ __forceinline__ double far_group(const double* __restrict__ mt, int nFar, double cq, double slMid,
                                            double d, int lane, const double* __restrict__ e2tab) {
    double B[NB];
    // the first 64 maskers initialise the sums: every lane takes part, a lane past nFar (>= 1) with a zero term
    {
        const int m = min(lane, nFar - 1);
        const double I = mt[4 * m], zm = mt[4 * m + 1], sl = mt[4 * m + 2];
        double term = (lane < nFar) ? I * exp2_tab64<T>(sl, cq - zm, e2tab) : 0.0;   // cq - zm > 0 for m < nFar
        const double da = (sl - slMid) * (0.6931471805599453094 / T);              // slope offset in nats per Bark
#pragma unroll
        for (int j = 0; j <= J; ++j) {
            B[j] = term;
            term *= da;
        }
#pragma unroll
        for (int j = J + 1; j < NB; ++j) B[j] = 0.0;
    }
    for (int m = lane + kWave; m < nFar; m += kWave) {
        const double I = mt[4 * m], zm = mt[4 * m + 1], sl = mt[4 * m + 2];
        double term = I * exp2_tab64<T>(sl, cq - zm, e2tab);
        const double da = (sl - slMid) * (0.6931471805599453094 / T);
#pragma unroll
        for (int j = 0; j <= J; ++j) {
            B[j] += term;
            term *= da;
        }
    }
    // 1/j! goes onto the per-lane partial sums: the wave totals come back as scalars, and a scalar times a constant
    // would need a register copy first
#pragma unroll
    for (int j = 2; j <= J; ++j) B[j] *= kInvFactorial[j];
    wave_sum_all<NB>(B, lane);
    double p = B[J];
#pragma unroll
    for (int j = J - 1; j >= 0; --j) p = fma(p, d, B[j]);
    return p * exp2_tab64<T>(slMid, d, e2tab);
}

// ---- Slope nodes: the upper-side sum of a whole frame from R prefix sums over the maskers (round 4).
// U_k = sum_{m < nUp_k} I_m 2^(s_m (zq_k - z_m)), zq_k = z_k - 1/2, is a sum of exponentials in the line's Bark value whose
// rates s_m differ from masker to masker -- which is why the lower side (one rate for all) is a suffix sum and this side was
// not.  Interpolating 2^(s d) in the SLOPE at R equispaced nodes sigma_r = sigma_0 - r h (Lagrange weights lambda_r(s_m)) turns
// it into R sums with one rate each:
//     U_k ~= sum_r 2^(sigma_r zq_k) Q_r[nUp_k],     Q_r[n] = sum_{m < n} lambda_r(s_m) I_m 2^(-sigma_r z_m),
// and because the nodes are equispaced, 2^(sigma_r zq) = E0 g^r with E0 = 2^(sigma_0 zq), g = 2^(-h zq): two 2^x and one
// Horner pass over R prefix sums per LINE (the masker side likewise: 2^(-sigma_0 z_m) and 2^(h z_m)), instead of one 2^x per
// (masker, line) pair near the line and an order-16 expansion per chunk far from it.  The nodes span the frame's own slope
// range [min s, max s] plus kNodeMargin spacings on either side (Lagrange interpolation on equispaced nodes is only well
// behaved away from the ends).  The prefix sums are kept for every fourth masker (a row per quad of lanes of the waves that
// compute the terms: <= 78 rows x 18 columns fit where the peak bins and the Bark grid were); the <= 3 maskers between a
// line's row and its nUp are added as direct pairs.
// Error, per line (DESIGN.md section 4 has the derivation): interpolation <= psi* sum_{m < nUp} I_m |prod_r (theta_m - r)| / R!
// with theta_m = (sigma_0 - s_m) / h and psi* = (h R / |sigma_0|)^R e^-R the maximum over the distance of
// (h d ln2)^R 2^(sigma_0 d) (column R of Q carries the sum); rounding <= K eps E0 sum_{m < nUp} Lambda_m I_m 2^(-sigma_0 z_m),
// Lambda_m = sum_r |lambda_r| (column R + 1).  A chunk one of whose lines has  bound > kNodeTol x (its total masked
// intensity)  is evaluated again by the sorted sweep (upper_cold): lines that live on distant loud maskers (beyond a cliff in
// the spectrum) are where the interpolation is weakest.  Frames whose slope range is too wide for R nodes, with fewer than
// kNodeMinMaskers or more than node_max_maskers(DIM) maskers take the sorted sweep as a whole.
constexpr int kNodeR = 16;
constexpr int kNodeMargin = 1;
constexpr int kNodeCols = kNodeR + 2;
constexpr double kNodeHMax = 0.22;                   // node spacing, bit per Bark: the frame's slope range <= 13 x 0.22 = 2.86
constexpr double kNodeHMin = 1e-3;
constexpr int kNodeMinMaskers = 32;
constexpr int kNodeC = 4;                            // maskers per row of the prefix sums (a quad of lanes)
constexpr int kNodeScanSegs = 7;                     // the scan over the rows: two waves, nine columns each, seven lanes per column
constexpr int kNodeSeg = 11;                         // ... rows per lane (78 rows / 7 lanes)
constexpr double kNodeTol = 1e-13;                   // accepted bound on the error of a line's masked intensity (relative)
constexpr double kNodeRoundEps = 8.0 * 0x1p-53;      // K eps: K = 8 covers the measured rounding (tools/rank_proto2.py: <= 1.1)
constexpr double kExpMinus16 = 1.1253517471925912e-07;
static_assert(kNodeR == 16, "psi* below is written for R = 16");
struct NodeWeights { double c[kNodeR]; };
constexpr NodeWeights make_node_weights() {          // 1 / prod_{j != r} (r - j) = (-1)^(R-1-r) / (r! (R-1-r)!)
    NodeWeights w{};
    for (int r = 0; r < kNodeR; ++r) {
        double f = 1.0;
        for (int j = 2; j <= r; ++j) f *= j;
        for (int j = 2; j <= kNodeR - 1 - r; ++j) f *= j;
        w.c[r] = (((kNodeR - 1 - r) & 1) ? -1.0 : 1.0) / f;
    }
    return w;
}
constexpr NodeWeights kNodeW = make_node_weights();

// Slope nodes, one line: U = E0 Horner_g(row[0 .. R-1]) + the NREM maskers between the line's row and its nUp as direct pairs
// (rem <= NREM of them count).  NREM is a template parameter so that the pairs' loads and the row's are all in flight together
// (a loop with an early exit serialises two dependent LDS round trips per pair).  The Horner pass runs as two chains in g^2.
template <int NREM, int TAB>
__device__ __forceinline__ double node_line(const double* __restrict__ row, const double* __restrict__ mt,
                                            const double* __restrict__ e2tab, int mBase, int rem, int mLast, double zq,
                                            double E0, double g) {
    double I[NREM > 0 ? NREM : 1], zm[NREM > 0 ? NREM : 1], sl[NREM > 0 ? NREM : 1];
#pragma unroll
    for (int j = 0; j < NREM; ++j) {
        const int m = min(mBase + j, mLast);
        I[j] = mt[4 * m]; zm[j] = mt[4 * m + 1]; sl[j] = mt[4 * m + 2];
    }
    const double g2 = g * g;
    double ev = row[kNodeR - 2], od = row[kNodeR - 1];
#pragma unroll
    for (int r = kNodeR - 4; r >= 0; r -= 2) {
        ev = fma(ev, g2, row[r]);
        od = fma(od, g2, row[r + 1]);
    }
    double up = fma(od, g, ev) * E0;
#pragma unroll
    for (int j = 0; j < NREM; ++j) up = fma(j < rem ? I[j] : 0.0, exp2_tab64<TAB>(sl[j], zq - zm[j], e2tab), up);
    return up;
}

// Sorted sweep, far field of chunk c: maskers [0, nFar) lie more than 1/2 Bark below EVERY line of the chunk; their sum is
// evaluated by far_group() for the whole chunk (one group) or its two halves.  The expansion is in (slope - middle slope of
// the frame) x (distance from the group's centre): the order follows from half the slope range times half the Bark span, so a
// frame of similar maskers (noise) gets by with a low order even where 64 lines span more than a Bark, and a frame with a loud
// and a quiet region still qualifies at the top of the spectrum.  false: the chunk takes no far field.
template <int TAB, bool HAVE_FAR>
__device__ __forceinline__ bool far_eval(const double* __restrict__ mt, const double* __restrict__ e2tab,
                                         const double* __restrict__ zbG, int M, int c, int lane, int nFar, double z,
                                         double slMid, double spreadHalf, double* out) {
    if (!HAVE_FAR || nFar < kFarMinMaskers || (MRC_PROFILE_SKIP & 1)) return false;
    // the group geometry is wave-uniform: scalar loads of the chunk's first / middle / last Bark values
    const int kFirst = c * kWave;
    const double zFirst = zbG[kFirst], zLast = zbG[min(kFirst + kWave - 1, M - 1)];
    const double zHalfEnd = zbG[min(kFirst + kWave / 2 - 1, M - 1)], zHalfBeg = zbG[min(kFirst + kWave / 2, M - 1)];
    double need = spreadHalf * (0.5 * (zLast - zFirst));
    int nGroups = 1;
    if (need > kFarLimit16) {                     // (wave-uniform)
        need = spreadHalf * (0.5 * fmax(zHalfEnd - zFirst, zLast - zHalfBeg));
        nGroups = 2;
    }
    const int order = need <= kFarLimit8 ? 8 : need <= kFarLimit12 ? 12 : need <= kFarLimit16 ? 16 : 0;
    if (!order) return false;
    const int myGroup = (nGroups == 2) ? (lane >> 5) : 0;
    double acc = 0.0;
    for (int g = 0; g < nGroups; ++g) {
        const double cg = (nGroups == 1) ? 0.5 * (zFirst + zLast)
                                         : (g == 0 ? 0.5 * (zFirst + zHalfEnd) : 0.5 * (zHalfBeg + zLast));
        const double cq = cg - 0.5, d = z - cg;
        double p;
        if (order == 8) p = far_group<8, 9, TAB>(mt, nFar, cq, slMid, d, lane, e2tab);
        else if (order == 12) p = far_group<12, 16, TAB>(mt, nFar, cq, slMid, d, lane, e2tab);
        else if (order == 16) p = far_group<16, 17, TAB>(mt, nFar, cq, slMid, d, lane, e2tab);
        else p = 0.0;
        if (g == myGroup) acc = p;
    }
    *out = acc;
    return true;
}

// Sorted sweep, near field of a chunk: the maskers [mFirst, max nUp) one 2^x per (masker, line) pair, added to tot.  Lines the
// masker is not below (u = 0) get exactly I_m when they see it at all (m < cnt): the in-band sum of the chunk's tail then
// starts at max nUp.
template <int TAB>
__device__ __forceinline__ double near_eval(const double* __restrict__ mt, const double* __restrict__ e2tab, int nUp,
                                            int cnt, double zq, bool tookFar, double tot) {
    // both counts are non-decreasing in the line index: the chunk's bounds sit in its first and last lane
    const int mLow = __builtin_amdgcn_readfirstlane(cnt);                      // min cnt
    const int mExp = __builtin_amdgcn_readlane(nUp, kWave - 1);                // max nUp
    const int mPlain = min(mExp, mLow);
    const int mFirst = tookFar ? __builtin_amdgcn_readfirstlane(nUp) : 0;
    // some line of the chunk is above the masker's band, every line sees the masker.  Maskers below
    // nUp of the chunk's FIRST line are more than 1/2 Bark below every line: u > 0 without the clamp.
    {
        const int mPos = min(max(__builtin_amdgcn_readfirstlane(nUp), mFirst), mPlain);
        const int mStop = (MRC_PROFILE_SKIP & 2) ? 0 : mPlain;
#pragma unroll 4                                // (four pairs in flight per lane)
        for (int m = mFirst; m < min(mPos, mStop); ++m) {
            const double I = mt[4 * m], zm = mt[4 * m + 1], sl = mt[4 * m + 2];
            tot = fma(I, exp2_tab64<TAB>(sl, zq - zm, e2tab), tot);
        }
#pragma unroll 4
        for (int m = mPos; m < mStop; ++m) {
            const double I = mt[4 * m], zm = mt[4 * m + 1], sl = mt[4 * m + 2];
            const double u = fmax(zq - zm, 0.0);
            tot = fma(I, exp2_tab64<TAB>(sl, u, e2tab), tot);
        }
    }
    // same, but part of the chunk lies below the masker's band (only when the chunk spans > 1 Bark)
    for (int m = mPlain; m < ((MRC_PROFILE_SKIP & 4) ? 0 : mExp); ++m) {
        const double I = mt[4 * m], zm = mt[4 * m + 1], sl = mt[4 * m + 2];
        const double u = fmax(zq - zm, 0.0);
        tot = fma(m < cnt ? I : 0.0, exp2_tab64<TAB>(sl, u, e2tab), tot);
    }
    return tot;
}

// The sorted sweep's upper side for ONE chunk, out of line: where the slope-node evaluation sends a chunk back (rare)
template <int TAB>
__device__ __attribute__((noinline)) double upper_cold(const double* mt, const double* e2tab, const double* zbG, int M, int c,
                                                       int lane, int nUp, int cnt, double z, double slMid,
                                                       double spreadHalf) {
    double far = 0.0;
    const bool took = far_eval<TAB, true>(mt, e2tab, zbG, M, c, lane, __builtin_amdgcn_readfirstlane(nUp), z, slMid,
                                          spreadHalf, &far);
    return near_eval<TAB>(mt, e2tab, nUp, cnt, z - 0.5, took, took ? far : 0.0);
}

}  // namespace
}  // namespace mrc
