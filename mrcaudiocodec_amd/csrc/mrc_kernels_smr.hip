// smr_kernel -- psychoac.py:134-219 on gfx950: Hann window -> real FFT -> intensity spectrum -> tonal
// maskers (strict 3-point peaks, kept in bin order) -> masked threshold on the MDCT line grid ->
// SMR per scale-factor band (and the per-band max |X| the scale factors need).  One 256-thread workgroup per
// (frame, signal), any block shape; units are walked in an XCD-contiguous order.
//
// The cost is the spreading (psychoac.py:68-78,166-168): ~P maskers x N/2 lines of 10^x in float64
// (P ~ 257, N/2 = 1024 on white noise).  Two evaluation modes:
//
//  EXACT = true   the reference's expression, operation by operation, pow() per (masker, line), summed
//                 in masker order.  ~200 fp64 instructions per pair.
//  EXACT = false  (default) "sorted sweep".  Lines and maskers are both sorted in Bark, so for a line k
//                 the maskers split into three index ranges (found once per frame from the masker side):
//                   more than 1/2 Bark below the line: I_m * 2^(s_m (z_k - z_m - 1/2)), s_m the level-dependent
//                           upper slope.  FAR FIELD (maskers below every line of a 64-line chunk): expansion in
//                           (slope - middle slope of the frame) x (distance from the chunk centre), one 2^x per
//                           masker and chunk, order 8/12/16 chosen from a rigorous bound -- far_group().  NEAR
//                           FIELD: one table-driven 2^x per pair (exp2_tab64, 16 instructions);
//                   inside +-1/2 Bark: exactly I_m, as a difference of double-double prefix sums;
//                   more than 1/2 Bark above: the lower slope is the same -27 dB/Bark for every masker, so the sum
//                           factors into one table value per line times a suffix sum over maskers (exponents
//                           carried in double-double).
//                 The band maximum of SPL(line) - SPL(threshold) is taken on the RATIO of the two intensities and
//                 converted with one log10 per band.  Same integers as EXACT on every parity corpus, thresholds
//                 within 1e-10 dB (tests/test_gpu_parity.py::test_spread_modes_agree).
// DESIGN.md section 4 has the derivations, the error bounds and the measured instruction counts.
#include "mrc_smr_body.hpp"
#include "mrc_smr_short.hpp"

#include <algorithm>

namespace mrc {

// Two translation units.  The mono long-block kernel of the hot path -- smr_kernel<false, *, 256, 1024, 1>, 80 % of a
// headline step -- gains 3 % from LLVM's max-ILP scheduling strategy; the joint variant <..., 2> LOSES 2 % with it (more
// spills at the 128-register cap).  The strategy is a per-file option, so mrc_kernels_smr_mono.hip compiles that one
// instantiation (launch_smr_mono_long).  Every other instantiation of smr_kernel (mrc_smr_body.hpp) is compiled here, and
// smr_short_kernel (mrc_smr_short.hpp, launch_smr_short), which shares the math helpers only.

#ifdef MRC_NODE_STATS
extern "C" int mrc_debug_node_stats(unsigned long long* out4, int reset) {
    std::fill(out4, out4 + 4, 0ull);
    hipError_t e = smr_counters_take(gNodeStats, out4, reset);
    if (e == hipSuccess) e = smr_mono_node_stats_take(out4, reset);
    return e == hipSuccess ? 0 : -1;
}
#endif

#ifdef MRC_PROFILE_PHASES
extern "C" int mrc_debug_phase_cycles(unsigned long long* out32, int reset) {
    std::fill(out32, out32 + 32, 0ull);
    hipError_t e = smr_counters_take(gPhaseCycles, out32, reset);
    if (e == hipSuccess) e = smr_mono_phase_cycles_take(out32, reset);
    return e == hipSuccess ? 0 : -1;
}
#endif

bool smr_peaks_fit(const DevShape& S) {
    // peak bins p = 1 .. peakLast - 2 (psychoac.py:160), no two of them adjacent
    return (S.peakLast - 1) / 2 + 1 <= kWave * kSmrMaxSeg;
}

size_t smr_generic_lds_bytes(const DevShape& S) {
    size_t lds = 0;
    (void)smr_launch_layout(S, &lds);
    return lds;
}

hipError_t launch_smr(const DevShape& S, int64_t nFrames, const void* chL, const void* chR, int fmt, int64_t stride,
                      const int64_t* offsets, const double* lines, const int* oscale, double* smr, double* thresh,
                      double* bandPeak, const int* msSwitch, bool exactSpread, hipStream_t st, unsigned long long* sens) {
    if (nFrames <= 0) return hipSuccess;
    const int nsig = chR ? 4 : 1;
    const int H = S.H, M = S.halfN;
    size_t lds = 0;
    const SmrLds lay = smr_launch_layout(S, &lds);
    const dim3 grid((unsigned)(nFrames * nsig));
    const bool isLong = H == 1024 && M == 1024 && S.peakLast == 924 && lay.twOff >= 0;
    const bool isShort = H == 128 && M == 128 && S.peakLast == 28 && lay.twOff >= 0;
    const bool isTrans = H == 576 && M == 576 && S.peakLast == 476 && lay.twOff < 0;
    // the hot paths: mono, and (long blocks) joint stereo with the switch known; no thresholds wanted
    const int mode = (thresh || !bandPeak) ? 0 : (nsig == 1 && !msSwitch) ? 1 : (nsig == 4 && msSwitch) ? 2 : 0;
    // short blocks of the hot paths: a wavefront per unit
    if (isShort && !exactSpread && mode != 0 && S.nBands <= 32 && S.N == 256 && !sens)
        return launch_smr_short(S, nFrames * nsig, mode, chL, chR, fmt, stride, offsets, lines, oscale, smr, bandPeak, msSwitch, st);
    // the mono long block: the other unit's kernel
    if (isLong && !exactSpread && mode == 1)
        return launch_smr_mono_long(S, nFrames, chL, fmt, stride, offsets, lines, oscale, smr, bandPeak, st, sens);
    // blocks of up to 128 lines (two 64-line chunks) run as two-wave workgroups (no idle waves holding CU wave slots), all
    // others with 256 threads
#define MRC_SMR_LAUNCH(EX, TY, THREADS, LG, MD)                                                                      \
    hipLaunchKernelGGL((smr_kernel<EX, TY, THREADS, LG, MD>), grid, dim3(THREADS), lds, st, S, nsig, (const TY*)chL, \
                       (const TY*)chR, stride, offsets, lines, oscale, smr, thresh, bandPeak, msSwitch, lay, sens)
#define MRC_SMR_PICK(EX, TY) do { if (isShort && !EX && mode == 1) MRC_SMR_LAUNCH(EX, TY, 128, 128, 1);               \
                                  else if (isShort && !EX) MRC_SMR_LAUNCH(EX, TY, 128, 128, 0);                      \
                                  else if (M <= 2 * kWave) MRC_SMR_LAUNCH(EX, TY, 128, 0, 0);                        \
                                  else if (isLong && !EX && mode == 2) MRC_SMR_LAUNCH(EX, TY, 256, 1024, 2);         \
                                  else if (isLong && !EX) MRC_SMR_LAUNCH(EX, TY, 256, 1024, 0);                      \
                                  else if (isTrans && !EX && mode == 1) MRC_SMR_LAUNCH(EX, TY, 256, 576, 1);         \
                                  else if (isTrans && !EX) MRC_SMR_LAUNCH(EX, TY, 256, 576, 0);                      \
                                  else MRC_SMR_LAUNCH(EX, TY, 256, 0, 0); } while (0)
    if (fmt == kSampleI16) { if (exactSpread) MRC_SMR_PICK(true, short); else MRC_SMR_PICK(false, short); }
    else { if (exactSpread) MRC_SMR_PICK(true, double); else MRC_SMR_PICK(false, double); }
#undef MRC_SMR_PICK
#undef MRC_SMR_LAUNCH
    return hipGetLastError();
}

}  // namespace mrc
