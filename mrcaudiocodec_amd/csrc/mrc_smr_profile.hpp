// The build switches of smr_kernel's diagnostics, all in one place.  None belongs in a product library -- three of them
// make the kernel compute something else -- so each is refused unless the build also says -DMRC_PROFILING_BUILD:
//   MRC_PROFILE_SKIP=<mask>  (wrong results) sweep parts to leave out: 1 far field, 2 direct pairs, 4 partial pairs, 8 chunk tail
//   MRC_PROFILE_STOP=<n>     (wrong results) leave the kernel after phase n
//   MRC_PROFILE_PHASES       shader-clock cycles per kernel phase -> mrc_debug_phase_cycles (tools/phase_profile.py)
//   MRC_NODE_STATS           how many units / chunks took which evaluation -> mrc_debug_node_stats (tools/node_stats.py)
// The counters are device globals of the unit that includes this header (one copy per translation unit: device code is
// linked per unit); smr_counters_take adds a unit's copy to the caller's totals, and mrc_kernels_smr_mono.hip exports its own.
#pragma once
#include <hip/hip_runtime.h>

#if (defined(MRC_PROFILE_SKIP) || defined(MRC_PROFILE_STOP) || defined(MRC_PROFILE_PHASES) || defined(MRC_NODE_STATS)) && \
    !defined(MRC_PROFILING_BUILD)
#error "MRC_PROFILE_SKIP / MRC_PROFILE_STOP / MRC_PROFILE_PHASES / MRC_NODE_STATS need -DMRC_PROFILING_BUILD: not for a product library"
#endif

#ifndef MRC_PROFILE_SKIP
#define MRC_PROFILE_SKIP 0
#endif
#ifdef MRC_PROFILE_STOP
#define MRC_STOP(i) do { if (MRC_PROFILE_STOP == (i)) return; } while (0)
#else
#define MRC_STOP(i) do { } while (0)
#endif

namespace mrc {
namespace {

#ifdef MRC_NODE_STATS
__device__ unsigned long long gNodeStats[4];     // units with nodes, units without, chunks by nodes, chunks sent back
#define MRC_NODE_COUNT(i) do { if (lane == 0) atomicAdd(&gNodeStats[i], 1ull); } while (0)
#else
#define MRC_NODE_COUNT(i) do { } while (0)
#endif

#ifdef MRC_PROFILE_PHASES
// summed over the waves of every 64th workgroup (per workgroup in LDS, flushed once at its end: an atomic to global memory
// per marker from every wave made the build sixteen times slower than the kernel it was meant to describe)
__device__ unsigned long long gPhaseCycles[32];
#define MRC_PHASE(i)                                                                  \
    do {                                                                              \
        const long long now_ = __builtin_readcyclecounter();                          \
        if (lane == 0) atomicAdd(&sPhase_[i], (unsigned long long)(now_ - tPhase_));  \
        tPhase_ = __builtin_readcyclecounter();                                       \
    } while (0)
#else
#define MRC_PHASE(i) do { } while (0)
#endif

}  // namespace

#if defined(MRC_NODE_STATS) || defined(MRC_PROFILE_PHASES)
namespace {
// out[0 .. N) += this unit's copy of a counter array (after the device is idle); reset: clear the copy
template <int N>
hipError_t smr_counters_take(unsigned long long (&counters)[N], unsigned long long* out, int reset) {
    unsigned long long v[N] = {}, zero[N] = {};
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpyFromSymbol(v, HIP_SYMBOL(counters), sizeof v);
    if (e == hipSuccess && reset) e = hipMemcpyToSymbol(HIP_SYMBOL(counters), zero, sizeof zero);
    for (int i = 0; i < N; ++i) out[i] += v[i];
    return e;
}
}  // namespace
hipError_t smr_mono_node_stats_take(unsigned long long* out4, int reset);       // (MRC_NODE_STATS)
hipError_t smr_mono_phase_cycles_take(unsigned long long* out32, int reset);    // (MRC_PROFILE_PHASES)
#endif

}  // namespace mrc
