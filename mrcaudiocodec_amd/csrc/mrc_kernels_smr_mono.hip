// The mono long-block instantiation of smr_kernel (psychoac.py:134-219 for one channel of a 1024 + 1024 block, the hot
// path's dominant kernel) as a translation unit of its own, so that it can be compiled with LLVM's max-ILP scheduling
// strategy (Makefile: SMR_MONO_SCHED), which this instantiation gains 3 % from and the joint one loses 2 % with.
// This unit defines launch_smr_mono_long only (diagnostics builds: and the readers of its copy of the counters).
#include "mrc_smr_body.hpp"

namespace mrc {

hipError_t launch_smr_mono_long(const DevShape& S, int64_t nFrames, const void* chL, int fmt, int64_t stride,
                                const int64_t* offsets, const double* lines, const int* oscale, double* smr,
                                double* bandPeak, hipStream_t st, unsigned long long* sens) {
    size_t lds = 0;
    const SmrLds lay = smr_launch_layout(S, &lds);
    const dim3 grid((unsigned)nFrames);
    if (fmt == kSampleI16)
        hipLaunchKernelGGL((smr_kernel<false, short, 256, 1024, 1>), grid, dim3(256), lds, st, S, 1, (const short*)chL,
                           (const short*)nullptr, stride, offsets, lines, oscale, smr, (double*)nullptr, bandPeak,
                           (const int*)nullptr, lay, sens);
    else
        hipLaunchKernelGGL((smr_kernel<false, double, 256, 1024, 1>), grid, dim3(256), lds, st, S, 1, (const double*)chL,
                           (const double*)nullptr, stride, offsets, lines, oscale, smr, (double*)nullptr, bandPeak,
                           (const int*)nullptr, lay, sens);
    return hipGetLastError();
}

#ifdef MRC_NODE_STATS
hipError_t smr_mono_node_stats_take(unsigned long long* out4, int reset) { return smr_counters_take(gNodeStats, out4, reset); }
#endif
#ifdef MRC_PROFILE_PHASES
hipError_t smr_mono_phase_cycles_take(unsigned long long* out32, int reset) { return smr_counters_take(gPhaseCycles, out32, reset); }
#endif

}  // namespace mrc
