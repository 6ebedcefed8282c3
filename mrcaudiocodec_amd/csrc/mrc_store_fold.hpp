// What the output kernels of the store's window calls share (mrc_kernels_store.hip, mrc_kernels_store_span.hip): the tile
// sizes, the polyphase fold of one output from a staged run, and the read-ahead of the sums.  Device code, internal to each unit.
#pragma once
#include "mrc_device.hpp"

namespace mrc {
using namespace dev;
namespace {

constexpr int kWindowThreads = 256;

constexpr int kResampleThreads = 256, kResampleWave = 64;
constexpr int kResampleRun = 4089;                                   // doubles a workgroup stages at most: 255 * 8 + 2 * 1024 + 1
constexpr int kResampleLds = kResampleRun + kResampleRun / 32 + 1;   // ... with one double of padding per 32 (skew)

__device__ inline int64_t floor_div(int64_t a, int64_t b) {         // b > 0
    const int64_t q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// (Taps: a pointer to const double -- the kernel argument of the single-ratio kernels, or GlobalTaps where the pointer was read
// out of memory and the compiler has to be told the address space that it sees for itself in a kernel argument)
using GlobalTaps = const __attribute__((address_space(1))) double*;

// v = the left fold from +0.0 over j ascending of taps[j][p] * run[first + j], every product rounded once, then added.
// kUp: 1 or 2 -- `up` itself: a tap's row is read at addresses the whole wave shares (scalar loads) and the lane picks its
// phase's -- or 0: any `up`, each lane loads taps[j][p].  kSkew: the run's layout.  Eight taps and samples are read ahead of
// their eight additions.
template <int kUp, bool kSkew, class Taps>
__device__ inline double resample_fold(Taps __restrict__ taps, int up, int p, const double* run, int first, int nTaps) {
    const auto tap = [&](int j) {
        if (kUp == 1) return taps[j];
        if (kUp == 2) {
            const double c0 = taps[2 * j], c1 = taps[2 * j + 1];
            return p ? c1 : c0;
        }
        return taps[(int64_t)j * up + p];
    };
    const auto at = [](int i) { return kSkew ? i + (i >> 5) : i; };
    double acc = 0.0;
    int j = 0;
    for (; j + 8 <= nTaps; j += 8) {
        double c[8], y[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            c[u] = tap(j + u);
            y[u] = run[at(first + j + u)];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = __dadd_rn(acc, __dmul_rn(c[u], y[u]));
    }
    for (; j < nTaps; ++j) acc = __dadd_rn(acc, __dmul_rn(tap(j), run[at(first + j)]));
    return acc;
}
template <bool kSkew, class Taps>
__device__ inline double resample_fold_up(Taps __restrict__ taps, int up, int p, const double* run, int first, int nTaps) {
    return up == 1 ? resample_fold<1, kSkew>(taps, up, p, run, first, nTaps)
         : up == 2 ? resample_fold<2, kSkew>(taps, up, p, run, first, nTaps)
                   : resample_fold<0, kSkew>(taps, up, p, run, first, nTaps);
}

constexpr int kSumAhead = 4;                                         // terms whose samples are loaded ahead of their additions

}  // namespace
}  // namespace mrc
