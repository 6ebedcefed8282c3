// The store's folding output kernels for terms with SPANS (mrc_pac_store_decode_window_spans, mrc_api_store.cpp): kernels beside
// sum_out_kernel, resample_sum_out_kernel and resample_multi_sum_out_kernel (mrc_kernels_store.hip, which describes rows, tiles,
// the lane-to-output map, the staged run and the fold they share), in a unit of their own so that those stay as compiled.
//
//   span_sum_out_kernel, span_resample_sum_out_kernel, span_resample_multi_sum_out_kernel   the three folding kernels
//     where a term sounds only inside a SPAN of the row and may fade at either end (mrc_pac_store_decode_window_spans).  A
//     TermSpan (first, len, fadeIn, fadeOut, origin) lies beside each SumTerm, read at the same workgroup-wide address.  With
//     j = t - first the term is silent for j < 0 or j >= len -- it adds nothing -- and else gives e * v, e the half-sample
//     linear ramp (2 j + 1) / (2 fadeIn) or (2 (len - 1 - j) + 1) / (2 fadeOut), one __ddiv_rn of two exact integers and one
//     __dmul_rn, and v itself between the ramps; gain, the order of the terms and the formats are the kernels' above.  The gate
//     is not only the meaning: the host synthesised the term's planes for its span alone (the plane's sample 2 L is row sample
//     `origin`, not 0), so what lies beside the span in the plane is half an overlap-add and is never loaded.
//     span_sum_out_kernel: a thread loads a term's sample only inside the span, four terms ahead as sum_out_kernel.
//     The two LDS kernels: a tile stages a term's run and takes its barrier pair only where its 256 outputs meet the span --
//     tested on blockIdx, the loop counter and the record alone, so the whole workgroup branches together around
//     __syncthreads -- and the run is that of the outputs inside the span, so it never leaves what was synthesised.  A row
//     of K abutting pieces costs one or two staged terms per tile, not K.  No atomics, no scratch.
//
#include "mrc_store_fold.hpp"

namespace mrc {
using namespace dev;
namespace {

// the envelope of a span applied to v at j = t - first, 0 <= j < len: one division of two exact integers and one product on a
// ramp, v itself between the ramps (fadeIn + fadeOut <= len: at most one ramp holds)
__device__ inline double span_shape(const TermSpan& sp, int64_t j, double v) {
    if (j < sp.fadeIn) return __dmul_rn(__ddiv_rn((double)(2 * j + 1), (double)(2 * sp.fadeIn)), v);
    if (j >= sp.len - sp.fadeOut) return __dmul_rn(__ddiv_rn((double)(2 * (sp.len - 1 - j) + 1), (double)(2 * sp.fadeOut)), v);
    return v;
}

// sum_term_sample under a span: +0.0 outside it, WITHOUT a load -- the plane was planned for the span, what lies beside it is
// half an overlap-add or another term's -- and the shaped sample inside.  t < window; the plane's sample 2 L is row sample origin.
__device__ inline double span_term_sample(const SumTerm& tm, const TermSpan& sp, int c, int64_t t, int64_t planeLen, int L,
                                          const double* __restrict__ planes) {
    const int64_t j = t - sp.first;
    if (j < 0 || j >= sp.len) return 0.0;
    const int64_t tp = t - sp.origin, pos = tm.w.start + tp;         // (0 <= tp < the planned length <= planeLen - 4 L)
    double y = 0.0;
    if (pos >= 0 && pos < tm.w.nSamples && tp >= 0 && tp < planeLen - 2 * (int64_t)L)
        y = planes[tm.w.plane + (int64_t)(tm.w.nch == 2 ? c : 0) * planeLen + 2 * (int64_t)L + tp];
    return span_shape(sp, j, y);
}

__global__ __launch_bounds__(kWindowThreads) void span_sum_out_kernel(const SumTerm* __restrict__ terms,
                                                                      const TermSpan* __restrict__ spans,
                                                                      const long long* __restrict__ termOffset, int64_t window,
                                                                      int64_t tiles, int nchOut, int format, int L, int64_t planeLen,
                                                                      const double* __restrict__ planes, void* __restrict__ out) {
    const int64_t row = (int64_t)blockIdx.x / tiles;                 // item * nchOut + channel
    const int64_t t = ((int64_t)blockIdx.x - row * tiles) * kWindowThreads + threadIdx.x;
    const int64_t k = row / nchOut;
    const int c = (int)(row - k * nchOut);
    const int64_t jEnd = termOffset[k + 1];
    int64_t j = termOffset[k];
    if (t >= window) return;
    // a silent term's sample is +0.0: gain * +0.0 added to a fold that began at +0.0 leaves its bits, so it "adds nothing"
    double acc = 0.0;
    for (; j + kSumAhead <= jEnd; j += kSumAhead) {
        double g[kSumAhead], y[kSumAhead];
#pragma unroll
        for (int u = 0; u < kSumAhead; ++u) {
            g[u] = terms[j + u].gain;
            y[u] = span_term_sample(terms[j + u], spans[j + u], c, t, planeLen, L, planes);
        }
#pragma unroll
        for (int u = 0; u < kSumAhead; ++u) acc = __dadd_rn(acc, __dmul_rn(g[u], y[u]));
    }
    for (; j < jEnd; ++j) acc = __dadd_rn(acc, __dmul_rn(terms[j].gain, span_term_sample(terms[j], spans[j], c, t, planeLen, L, planes)));
    store_window_value(out, row * window + t, format, acc);
}

// One resampled term of a tile under its span, the body the two LDS kernels below share: outputs [a0, a1) of the row are the
// tile's that lie in the span (a0 < a1, the same for the whole workgroup); their run of intermediate samples is staged -- it
// lies inside what the planner had synthesised for the span -- and thread t folds and shapes its output between the barriers.
template <class Taps>
__device__ inline void span_resampled_term(const SumTerm& tm, const TermSpan& sp, int64_t a0, int64_t a1, int64_t t, int c, int L,
                                           int64_t planeLen, int up, int down, int W, int skew, Taps taps,
                                           const double* __restrict__ planes, double* run, double* acc) {
    const int64_t n0 = tm.outStart + a0, nLast = tm.outStart + a1 - 1;
    const int64_t qFirst = floor_div(n0 * down, up) - W + 1;
    const int len = (int)(floor_div(nLast * down, up) + W - qFirst + 1);       // <= kResampleRun (the launcher's check)
    const double* plane = planes + tm.w.plane + (int64_t)(tm.w.nch == 2 ? c : 0) * planeLen;
    for (int i = threadIdx.x; i < len; i += kResampleThreads) {
        const int64_t m = qFirst + i, at = 2 * (int64_t)L + (m - tm.w.start);
        double v = 0.0;
        if (m >= 0 && m < tm.w.nSamples && at >= 0 && at < planeLen) v = plane[at];
        run[i + skew * (i >> 5)] = v;
    }
    __syncthreads();
    if (t >= a0 && t < a1) {
        const int64_t nd = (tm.outStart + t) * down, q = floor_div(nd, up);
        const int p = (int)(nd - q * up), first = (int)(q - W + 1 - qFirst);
        const double v = skew ? resample_fold_up<true>(taps, up, p, run, first, 2 * W) : resample_fold_up<false>(taps, up, p, run, first, 2 * W);
        *acc = __dadd_rn(*acc, __dmul_rn(tm.gain, span_shape(sp, t - sp.first, v)));
    }
    __syncthreads();                                                 // (the next term's run goes over this one)
}

__global__ __launch_bounds__(kResampleThreads) void span_resample_sum_out_kernel(const SumTerm* __restrict__ terms,
                                                                                 const TermSpan* __restrict__ spans,
                                                                                 const long long* __restrict__ termOffset,
                                                                                 int64_t window, int64_t tiles, int nchOut, int format,
                                                                                 int L, int64_t planeLen, int up, int down, int W,
                                                                                 int evenOdd, int skew, const double* __restrict__ taps,
                                                                                 const double* __restrict__ planes,
                                                                                 void* __restrict__ out) {
    __shared__ double run[kResampleLds];
    const int64_t row = (int64_t)blockIdx.x / tiles;                 // item * nchOut + channel
    const int64_t t0 = ((int64_t)blockIdx.x - row * tiles) * kResampleThreads;
    const int64_t k = row / nchOut;
    const int c = (int)(row - k * nchOut);
    const int lane = threadIdx.x % kResampleWave, wave = threadIdx.x / kResampleWave;      // (resample_out_kernel's map)
    const int64_t t = t0 + wave * kResampleWave + (evenOdd ? 2 * (lane & 31) + (lane >> 5) : lane);
    const int64_t tEnd = min(t0 + kResampleThreads, window), jEnd = termOffset[k + 1];
    double acc = 0.0;
    for (int64_t j = termOffset[k]; j < jEnd; ++j) {                 // (every branch on the term or its span: the whole workgroup)
        const SumTerm tm = terms[j];
        const TermSpan sp = spans[j];
        // the tile's outputs inside the span, from blockIdx, the loop counter and the record alone: a term that the tile does
        // not meet stages nothing and takes no barrier
        const int64_t a0 = max((int64_t)sp.first, t0), a1 = min((int64_t)(sp.first + sp.len), tEnd);
        if (tm.w.nSamples == 0 || a0 >= a1) continue;
        span_resampled_term(tm, sp, a0, a1, t, c, L, planeLen, up, down, W, skew, taps, planes, run, &acc);
    }
    if (t < window) store_window_value(out, row * window + t, format, acc);
}

__global__ __launch_bounds__(kResampleThreads) void span_resample_multi_sum_out_kernel(const SumTerm* __restrict__ terms,
                                                                                       const TermSpan* __restrict__ spans,
                                                                                       const int* __restrict__ ratioOf,
                                                                                       const SpeedRatio* __restrict__ ratios,
                                                                                       const long long* __restrict__ termOffset,
                                                                                       int64_t window, int64_t tiles, int nchOut,
                                                                                       int format, int L, int64_t planeLen,
                                                                                       const double* __restrict__ planes,
                                                                                       void* __restrict__ out) {
    __shared__ double run[kResampleLds];
    const int64_t row = (int64_t)blockIdx.x / tiles;                 // item * nchOut + channel
    const int64_t t0 = ((int64_t)blockIdx.x - row * tiles) * kResampleThreads;
    const int64_t k = row / nchOut;
    const int c = (int)(row - k * nchOut);
    const int64_t t = t0 + threadIdx.x;                              // the natural map, as in resample_multi_sum_out_kernel
    const int64_t tEnd = min(t0 + kResampleThreads, window), jEnd = termOffset[k + 1];
    double acc = 0.0;
    for (int64_t j = termOffset[k]; j < jEnd; ++j) {                 // (every branch on the term, its span or its ratio: the whole workgroup)
        const SumTerm tm = terms[j];
        const TermSpan sp = spans[j];
        const int64_t a0 = max((int64_t)sp.first, t0), a1 = min((int64_t)(sp.first + sp.len), tEnd);
        if (tm.w.nSamples == 0 || a0 >= a1) continue;                // no plane, or the tile does not meet the span
        const SpeedRatio r = ratios[ratioOf[j]];                     // (blockIdx and the loop counter alone: scalar)
        if (r.W == 0) {                                              // the unit ratio: span_sum_out_kernel's term, no LDS, no barrier
            if (t < window) acc = __dadd_rn(acc, __dmul_rn(tm.gain, span_term_sample(tm, sp, c, t, planeLen, L, planes)));
            continue;
        }
        span_resampled_term(tm, sp, a0, a1, t, c, L, planeLen, r.up, r.down, r.W, r.skew, (GlobalTaps)r.taps, planes, run, &acc);
    }
    if (t < window) store_window_value(out, row * window + t, format, acc);
}

}  // namespace

hipError_t launch_span_sum_out(int64_t nRows, const SumTerm* terms, const TermSpan* spans, const long long* termOffset,
                               int64_t window, int nchOut, int format, int L, int64_t planeLen, const double* planes, void* out,
                               hipStream_t st) {
    if (nRows <= 0 || window <= 0) return hipSuccess;
    const int64_t tiles = (window + kWindowThreads - 1) / kWindowThreads;
    const int64_t blocks = tiles * nRows * nchOut;
    if (blocks > 0x7fffffffLL || !spans || planeLen < 4 * (int64_t)L) return hipErrorInvalidValue;
    hipLaunchKernelGGL(span_sum_out_kernel, dim3((unsigned)blocks), dim3(kWindowThreads), 0, st, terms, spans, termOffset, window,
                       tiles, nchOut, format, L, planeLen, planes, out);
    return hipGetLastError();
}

hipError_t launch_span_resample_sum_out(int64_t nRows, const SumTerm* terms, const TermSpan* spans, const long long* termOffset,
                                        int64_t window, int nchOut, int format, int L, int64_t planeLen, int up, int down, int W,
                                        int evenOdd, int skew, const double* taps, const double* planes, void* out, hipStream_t st) {
    if (nRows <= 0 || window <= 0) return hipSuccess;
    const int64_t tiles = (window + kResampleThreads - 1) / kResampleThreads;
    const int64_t blocks = tiles * nRows * nchOut;
    if (blocks > 0x7fffffffLL || !spans || planeLen < 4 * (int64_t)L || up < 1 || down < 1 || W < 1 ||
        ((int64_t)(kResampleThreads - 1) * down + up - 1) / up + 2 * (int64_t)W + 1 > kResampleRun)
        return hipErrorInvalidValue;                                 // (a run that would not fit the workgroup's LDS)
    hipLaunchKernelGGL(span_resample_sum_out_kernel, dim3((unsigned)blocks), dim3(kResampleThreads), 0, st, terms, spans, termOffset,
                       window, tiles, nchOut, format, L, planeLen, up, down, W, evenOdd, skew, taps, planes, out);
    return hipGetLastError();
}

hipError_t launch_span_resample_multi_sum_out(int64_t nRows, const SumTerm* terms, const TermSpan* spans, const int* ratioOf,
                                              const SpeedRatio* ratios, const SpeedRatio* ratiosHost, int nRatios,
                                              const long long* termOffset, int64_t window, int nchOut, int format, int L,
                                              int64_t planeLen, const double* planes, void* out, hipStream_t st) {
    if (nRows <= 0 || window <= 0) return hipSuccess;
    const int64_t tiles = (window + kResampleThreads - 1) / kResampleThreads;
    const int64_t blocks = tiles * nRows * nchOut;
    if (blocks > 0x7fffffffLL || !spans || nRatios < 1 || !ratiosHost || planeLen < 4 * (int64_t)L) return hipErrorInvalidValue;
    for (int i = 0; i < nRatios; ++i) {
        const SpeedRatio& r = ratiosHost[i];
        if (r.W == 0) continue;                                      // the unit ratio: no run
        if (r.up < 1 || r.down < 1 || r.W < 1 || !r.taps ||
            ((int64_t)(kResampleThreads - 1) * r.down + r.up - 1) / r.up + 2 * (int64_t)r.W + 1 > kResampleRun)
            return hipErrorInvalidValue;                             // (a run that would not fit the workgroup's LDS)
    }
    hipLaunchKernelGGL(span_resample_multi_sum_out_kernel, dim3((unsigned)blocks), dim3(kResampleThreads), 0, st, terms, spans, ratioOf,
                       ratios, termOffset, window, tiles, nchOut, format, L, planeLen, planes, out);
    return hipGetLastError();
}

}  // namespace mrc
