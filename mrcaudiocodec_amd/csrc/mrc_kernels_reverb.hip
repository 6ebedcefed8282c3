// Reverberation of the resident store's window terms (mrc_pac_store_decode_window_reverb, mrc_api_store.cpp): uniformly
// partitioned overlap-save convolution in float64, hop B = MRC_STORE_REVERB_BLOCK samples, transforms of N = 2 B points.
//
//   x      a term's dry signal, t = 0 at the term's OWN window start (the segments are anchored there and nowhere else: what a
//          workgroup computes depends on the term, its impulse response and t alone -- not on the slab, the row's place in the
//          call, the other terms, or the bank's other responses)
//   X_s    the forward transform of x[(s - 1) B .. (s + 1) B), s = -(P - 1) .. M - 1 (M = ceil(window / B) output blocks, P =
//          ceil(len(h) / B) partitions), zero where t lies outside [-(len(h) - 1), window): samples no output reads are not
//          loaded, so a longer pre-roll decoded for a neighbour's sake changes no bit
//   H_p    the forward transform of h[p B .. (p + 1) B) followed by B zeros, made ONCE per bank by the same kernel
//   y      block m, y[m B + u] for 0 <= u < B, is the last B samples of the inverse transform of sum_p X_{m - p} H_p: element
//          B + u of the circular convolution reads x_seg[B + u - j], j < B, which never wraps
//
// reverb_forward_kernel   one workgroup of 256 threads per (source, segment).  It loads N samples -- channel 0 as the real
//   part and, for a two-channel term, channel 1 as the imaginary part: h is real, so the two channels ride through one transform
//   and come apart again as the real and imaginary part of the inverse; a one-channel source leaves the imaginary part zero
//   (no real-input split) -- runs the Stockham passes of mrc_device.hpp (five of radix 4, one of radix 2) with the quadrant
//   twiddles staged in LDS, and writes the N bins to the slab's spectra.  A source record says where its samples lie, which of
//   them exist and how many a segment takes (N for a signal, B for a partition of h).
//
// reverb_fold_kernel   one workgroup per (row, output block).  It walks the row's terms in the order given.  An unconvolved
//   term adds gain * dry sample in the time domain: __dmul_rn then __dadd_rn from +0.0, sum_out_kernel's fold, so a row without
//   a convolved term is that kernel's bit for bit.  A convolved term accumulates Z = sum_p X[m - p] H[p], p ascending, eight bins
//   per thread in registers, stores conj(Z) to LDS, runs the same forward passes (the conjugate trick: the inverse is the
//   conjugate of the forward transform of the conjugate), scales by 1 / N (exact) and adds gain * y of the last B samples the same
//   way.  One inverse transform per convolved term: a term's y then depends on that term alone, and the row is the documented
//   fold over its terms whatever their kinds.  store_window_value converts the sum once.
//
// reverb_route_fold_kernel<G>   the fold of mrc_pac_store_decode_window_routed: one workgroup per (row, output block, group of
//   up to G output channels).  A term has ONE dry channel and a route record per output channel -- absent, dry, or a response
//   with the spectra of the term's source of that response's length.  Per channel the arithmetic is reverb_fold_kernel's,
//   expression for expression (the library is built without FMA contraction): the dry fold, Z = sum_p X[m - p] H[p] with p
//   ascending, ONE inverse transform per (term, channel), the gain's product rounded once, then added.  What the group shares
//   is the load of X: the channels of the group whose routes name the same source -- responses of one length -- walk the
//   partitions together, eight X bins per thread loaded once per partition for all of them.  A channel's bits depend on its
//   own routes alone, whatever shares its group.
//
// LDS: two buffers of N double2 and the twiddle quadrant, 72 KiB at N = 2048 -- two workgroups per CU, all three kernels.  No
// atomics; nothing depends on the grid.
#include "mrc_device.hpp"

namespace mrc {
using namespace dev;
namespace {

constexpr int kReverbThreads = 256;
constexpr int kB = MRC_STORE_REVERB_BLOCK, kN = 2 * kB;
constexpr int kBins = kN / kReverbThreads, kOuts = kB / kReverbThreads;      // per thread
static_assert(kN == 2048 || kN == 4096, "the pass list below is 2048 = 4^5 * 2 or 4096 = 4^6 (measurement builds: -DMRC_STORE_REVERB_BLOCK=2048)");

// the forward transform of A (LDS, natural order in, natural order out); returns the buffer that holds it
__device__ __forceinline__ double2* reverb_fft(double2* A, double2* B, const double2* wq, int tid) {
    const TwQuarter W{wq, kN / 4 - 1, 31 - __clz(kN / 4)};
    fft_pass<4, true, TwQuarter, kReverbThreads>(A, B, kN, 1, W, tid);
    __syncthreads();
    fft_pass<4, true, TwQuarter, kReverbThreads>(B, A, kN, 4, W, tid);
    __syncthreads();
    fft_pass<4, true, TwQuarter, kReverbThreads>(A, B, kN, 16, W, tid);
    __syncthreads();
    fft_pass<4, true, TwQuarter, kReverbThreads>(B, A, kN, 64, W, tid);
    __syncthreads();
    fft_pass<4, true, TwQuarter, kReverbThreads>(A, B, kN, 256, W, tid);
    __syncthreads();
    if constexpr (kN == 2048) fft_pass<2, true, TwQuarter, kReverbThreads>(B, A, kN, 1024, W, tid);
    else fft_pass<4, true, TwQuarter, kReverbThreads>(B, A, kN, 1024, W, tid);
    __syncthreads();
    return A;
}

__global__ __launch_bounds__(kReverbThreads) void reverb_forward_kernel(const ReverbSource* __restrict__ sources, int64_t maxSeg,
                                                                        const double* __restrict__ samples,
                                                                        const double2* __restrict__ twiddle,
                                                                        double2* __restrict__ spectra) {
    __shared__ double2 A[kN], Bf[kN], wq[kN / 4];
    const int tid = threadIdx.x;
    const int64_t k = (int64_t)blockIdx.x / maxSeg, seg = (int64_t)blockIdx.x - k * maxSeg;
    const ReverbSource src = sources[k];
    if (seg >= src.nSeg) return;                                     // (the whole workgroup)
    for (int i = tid; i < kN / 4; i += kReverbThreads) wq[i] = twiddle[i];
    const int64_t g0 = src.first + seg * kB;
#pragma unroll
    for (int q = 0; q < kBins; ++q) {
        const int i = tid + q * kReverbThreads;
        const int64_t g = g0 + i;
        double2 v = make_double2(0.0, 0.0);
        if (i < src.take && g >= src.lo && g < src.hi) {
            v.x = samples[src.re + g];
            if (src.im >= 0) v.y = samples[src.im + g];
        }
        A[i] = v;
    }
    __syncthreads();
    const double2* T = reverb_fft(A, Bf, wq, tid);
    double2* dst = spectra + (src.spec + seg) * kN;
#pragma unroll
    for (int q = 0; q < kBins; ++q) dst[tid + q * kReverbThreads] = T[tid + q * kReverbThreads];
}

__global__ __launch_bounds__(kReverbThreads) void reverb_fold_kernel(const ReverbTerm* __restrict__ terms,
                                                                     const long long* __restrict__ termOffset, int64_t window,
                                                                     int64_t blocks, int nch, int format, int64_t chStride,
                                                                     const double* __restrict__ dry,
                                                                     const double2* __restrict__ spectra,
                                                                     const double2* __restrict__ bank,
                                                                     const double2* __restrict__ twiddle, void* __restrict__ out) {
    __shared__ double2 A[kN], Bf[kN], wq[kN / 4];
    const int tid = threadIdx.x;
    const int64_t row = (int64_t)blockIdx.x / blocks, m = (int64_t)blockIdx.x - row * blocks;
    for (int i = tid; i < kN / 4; i += kReverbThreads) wq[i] = twiddle[i];
    // the row's terms: the same for the whole workgroup (indexed from blockIdx and the loop counter alone)
    const int64_t jEnd = termOffset[row + 1];
    double acc[kOuts][2];
#pragma unroll
    for (int q = 0; q < kOuts; ++q) acc[q][0] = acc[q][1] = 0.0;
    for (int64_t j = termOffset[row]; j < jEnd; ++j) {
        const ReverbTerm tm = terms[j];
        if (tm.spec < 0) {                                           // dry: sum_out_kernel's fold
#pragma unroll
            for (int q = 0; q < kOuts; ++q) {
                const int64_t t = m * kB + tid + q * kReverbThreads;
                if (t >= window) continue;
                for (int c = 0; c < nch; ++c) acc[q][c] = __dadd_rn(acc[q][c], __dmul_rn(tm.gain, dry[tm.dry + c * chStride + t]));
            }
            continue;
        }
        double2 z[kBins];
#pragma unroll
        for (int q = 0; q < kBins; ++q) z[q] = make_double2(0.0, 0.0);
        const double2* X = spectra + (tm.spec + m + tm.nPart - 1) * kN + tid;     // segment m - p: kN back per partition
        const double2* H = bank + tm.ir * kN + tid;
        for (int p = 0; p < tm.nPart; ++p, X -= kN, H += kN) {
            double2 x[kBins], h[kBins];
#pragma unroll
            for (int q = 0; q < kBins; ++q) {
                x[q] = X[q * kReverbThreads];
                h[q] = H[q * kReverbThreads];
            }
#pragma unroll
            for (int q = 0; q < kBins; ++q) {
                const double2 v = cmul(x[q], h[q]);
                z[q] = make_double2(z[q].x + v.x, z[q].y + v.y);
            }
        }
        __syncthreads();                                             // (the twiddles staged; the last term's reads of A done)
#pragma unroll
        for (int q = 0; q < kBins; ++q) A[tid + q * kReverbThreads] = make_double2(z[q].x, -z[q].y);
        __syncthreads();
        const double2* T = reverb_fft(A, Bf, wq, tid);
#pragma unroll
        for (int q = 0; q < kOuts; ++q) {
            const double2 v = T[kB + tid + q * kReverbThreads];
            acc[q][0] = __dadd_rn(acc[q][0], __dmul_rn(tm.gain, v.x * (1.0 / kN)));
            if (nch == 2) acc[q][1] = __dadd_rn(acc[q][1], __dmul_rn(tm.gain, -v.y * (1.0 / kN)));
        }
    }
#pragma unroll
    for (int q = 0; q < kOuts; ++q) {
        const int64_t t = m * kB + tid + q * kReverbThreads;
        if (t >= window) continue;
        for (int c = 0; c < nch; ++c) store_window_value(out, (row * nch + c) * window + t, format, acc[q][c]);
    }
}

// routes [term][C] (ReverbTerm: spec kRouteDry, kRouteNone or the source's first spectrum; .dry the term's one dry channel in
// every record); out [row][C][window]
template <int G>
__global__ __launch_bounds__(kReverbThreads) void reverb_route_fold_kernel(const ReverbTerm* __restrict__ routes,
                                                                           const long long* __restrict__ termOffset, int64_t window,
                                                                           int64_t blocks, int C, int groups, int format,
                                                                           const double* __restrict__ dry,
                                                                           const double2* __restrict__ spectra,
                                                                           const double2* __restrict__ bank,
                                                                           const double2* __restrict__ twiddle, void* __restrict__ out) {
    __shared__ double2 A[kN], Bf[kN], wq[kN / 4];
    const int tid = threadIdx.x;
    const int64_t cell = (int64_t)blockIdx.x / groups, row = cell / blocks, m = cell - row * blocks;
    const int c0 = (int)((int64_t)blockIdx.x - cell * groups) * G, nc = min(G, C - c0);      // channels [c0, c0 + nc): >= 1
    for (int i = tid; i < kN / 4; i += kReverbThreads) wq[i] = twiddle[i];
    const int64_t jEnd = termOffset[row + 1];
    double acc[G][kOuts];
#pragma unroll
    for (int i = 0; i < G; ++i)
#pragma unroll
        for (int q = 0; q < kOuts; ++q) acc[i][q] = 0.0;
    for (int64_t j = termOffset[row]; j < jEnd; ++j) {
        // the term's routes to the group's channels: the same for the whole workgroup
        ReverbTerm rt[G];
        bool anyDry = false;
#pragma unroll
        for (int i = 0; i < G; ++i) {
            rt[i] = routes[j * C + c0 + min(i, nc - 1)];
            if (i >= nc) rt[i].spec = kRouteNone;
            anyDry = anyDry || rt[i].spec == kRouteDry;
        }
        if (anyDry) {                                                // dry: sum_out_kernel's fold, the sample loaded once
#pragma unroll
            for (int q = 0; q < kOuts; ++q) {
                const int64_t t = m * kB + tid + q * kReverbThreads;
                if (t >= window) continue;
                const double v = dry[rt[0].dry + t];
#pragma unroll
                for (int i = 0; i < G; ++i)
                    if (rt[i].spec == kRouteDry) acc[i][q] = __dadd_rn(acc[i][q], __dmul_rn(rt[i].gain, v));
            }
        }
#pragma unroll
        for (int i = 0; i < G; ++i) {                                // wet: channel i leads the channels behind it on its source
            if (rt[i].spec < 0) continue;
            bool led = false;
#pragma unroll
            for (int e = 0; e < i; ++e) led = led || rt[e].spec == rt[i].spec;
            if (led) continue;                                       // (done with channel e)
            double2 z[G][kBins];
#pragma unroll
            for (int e = i; e < G; ++e)
#pragma unroll
                for (int q = 0; q < kBins; ++q) z[e][q] = make_double2(0.0, 0.0);
            const double2* X = spectra + (rt[i].spec + m + rt[i].nPart - 1) * kN + tid;     // segment m - p: kN back per partition
            for (int p = 0; p < rt[i].nPart; ++p, X -= kN) {
                double2 x[kBins];
#pragma unroll
                for (int q = 0; q < kBins; ++q) x[q] = X[q * kReverbThreads];
#pragma unroll
                for (int e = i; e < G; ++e) {
                    if (rt[e].spec != rt[i].spec) continue;          // (one source: one length, one nPart)
                    const double2* H = bank + (rt[e].ir + p) * kN + tid;
                    double2 h[kBins];
#pragma unroll
                    for (int q = 0; q < kBins; ++q) h[q] = H[q * kReverbThreads];
#pragma unroll
                    for (int q = 0; q < kBins; ++q) {
                        const double2 v = cmul(x[q], h[q]);
                        z[e][q] = make_double2(z[e][q].x + v.x, z[e][q].y + v.y);
                    }
                }
            }
#pragma unroll
            for (int e = i; e < G; ++e) {                            // one inverse transform per (term, channel)
                if (rt[e].spec != rt[i].spec) continue;
                __syncthreads();                                     // (the twiddles staged; the last reads of A done)
#pragma unroll
                for (int q = 0; q < kBins; ++q) A[tid + q * kReverbThreads] = make_double2(z[e][q].x, -z[e][q].y);
                __syncthreads();
                const double2* T = reverb_fft(A, Bf, wq, tid);
#pragma unroll
                for (int q = 0; q < kOuts; ++q) {
                    const double2 v = T[kB + tid + q * kReverbThreads];
                    acc[e][q] = __dadd_rn(acc[e][q], __dmul_rn(rt[e].gain, v.x * (1.0 / kN)));
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < G; ++i) {
        if (i >= nc) continue;
#pragma unroll
        for (int q = 0; q < kOuts; ++q) {
            const int64_t t = m * kB + tid + q * kReverbThreads;
            if (t < window) store_window_value(out, (row * C + c0 + i) * window + t, format, acc[i][q]);
        }
    }
}

}  // namespace

hipError_t launch_reverb_forward(int64_t nSources, int64_t maxSeg, const ReverbSource* sources, const double* samples,
                                 const double2* twiddle, double2* spectra, hipStream_t st) {
    if (nSources <= 0 || maxSeg <= 0) return hipSuccess;
    if (nSources > 0x7fffffffLL / maxSeg) return hipErrorInvalidValue;
    hipLaunchKernelGGL(reverb_forward_kernel, dim3((unsigned)(nSources * maxSeg)), dim3(kReverbThreads), 0, st, sources, maxSeg,
                       samples, twiddle, spectra);
    return hipGetLastError();
}

hipError_t launch_reverb_fold(int64_t nRows, const ReverbTerm* terms, const long long* termOffset, int64_t window, int nchOut,
                              int format, int64_t chStride, const double* dry, const double2* spectra, const double2* bank,
                              const double2* twiddle, void* out, hipStream_t st) {
    const int64_t blocks = (window + kB - 1) / kB;
    if (nRows <= 0 || blocks <= 0) return hipSuccess;
    if (nRows > 0x7fffffffLL / blocks) return hipErrorInvalidValue;
    hipLaunchKernelGGL(reverb_fold_kernel, dim3((unsigned)(nRows * blocks)), dim3(kReverbThreads), 0, st, terms, termOffset, window,
                       blocks, nchOut, format, chStride, dry, spectra, bank, twiddle, out);
    return hipGetLastError();
}

hipError_t launch_reverb_route_fold(int64_t nRows, const ReverbTerm* routes, const long long* termOffset, int64_t window,
                                    int nChannels, int group, int format, const double* dry, const double2* spectra,
                                    const double2* bank, const double2* twiddle, void* out, hipStream_t st) {
    const int64_t blocks = (window + kB - 1) / kB, groups = reverb_route_groups(nChannels, group);
    if (nRows <= 0 || blocks <= 0) return hipSuccess;
    if (nChannels < 1 || nRows > 0x7fffffffLL / (blocks * groups)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(nRows * blocks * groups)), threads(kReverbThreads);
    if (group == 1)
        hipLaunchKernelGGL(reverb_route_fold_kernel<1>, grid, threads, 0, st, routes, termOffset, window, blocks, nChannels, (int)groups,
                           format, dry, spectra, bank, twiddle, out);
    else if (group == 2)
        hipLaunchKernelGGL(reverb_route_fold_kernel<2>, grid, threads, 0, st, routes, termOffset, window, blocks, nChannels, (int)groups,
                           format, dry, spectra, bank, twiddle, out);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace mrc
