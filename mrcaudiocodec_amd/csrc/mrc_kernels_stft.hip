// Short-time Fourier transforms of the resident store's rows (mrc_pac_store_stft_window, mrc_api_store.cpp): complex bins,
// power, or the totals of a caller's filter bank over the power, in float64.
//
//   x      one channel of a row: L = (nFrames - 1) hop + nFft float64 samples, written by the existing rows call
//   X[m]   bins 0 .. nFft / 2 of frame m: sum_n g[n] x[m hop + n] e^{-2 pi i k n / nFft}.  The frame is real, so its transform is
//          ONE complex transform of H = nFft / 2 points of z[n] = g x[2 n] + i g x[2 n + 1] (every product rounded once) and a
//          pass that takes the even and the odd half apart: X[k] = (Z[k] + conj Z[H - k]) / 2 + w^k (Z[k] - conj Z[H - k]) / 2i,
//          w = e^{-2 pi i / nFft}.  No two frames share a transform: what comes out for frame m depends on that frame's nFft
//          samples and on nothing else -- not on its neighbours, the run it is in, the row's place in the slab or the grid.
//
// stft_kernel<NT>   one workgroup of 256 threads per (row, channel, run of F frames), F = stft_plan: a function of the
//   call's arguments alone.  It stages the run's span of the row, (F - 1) hop + nFft samples, in LDS once (at hop 160 and nFft 400
//   a sample is used 2.5 times), then transforms 256 / NT frames at a time, NT threads each: NT = 64 up to 512 points (a
//   200-point transform has 50 radix-4 butterflies -- one wave's worth), 128 up to 1024, 256 above, so that the transforms'
//   buffers never take more than 32 KiB.  The passes are mrc_device.hpp's Stockham passes of radix 4, 2, 3 and 5
//   (fft_pass_2345), twiddles from the nFft-point table in global memory at stride 2; all groups walk the same pass list, one
//   workgroup barrier between two passes.  Bins (or powers) of the run are assembled in LDS as [bin][frame] and leave as
//   runs along the frame axis, the fastest axis of every output layout.  MRC_STFT_BANK: one thread per (filter, frame)
//   folds w P over the filter's support in ascending k (__dmul_rn, __dadd_rn from +0.0) into the staging area, which is free by
//   then.  Power is __dadd_rn(__dmul_rn(re, re), __dmul_rn(im, im)).
//
// LDS: 32 KiB of transform buffers at most, 20.6 KiB of span, 20.6 KiB of assembly: 73.3 KiB, two workgroups per CU.  No atomics.
#include "mrc_device.hpp"

namespace mrc {
using namespace dev;
namespace {

constexpr int kStftThreads = 256;
constexpr int kStftMaxRun = 32;          // frames per workgroup at most
// float64 samples of a run's span (a single frame may take more: nFft <= 2048) and values of its assembled output: 2640 holds
// 12 frames of 201 bins at the odd stride 13 (three full rounds of four transforms) and 4 frames of 513 bins at stride 5 (two
// full rounds of two)
constexpr int kStftSpanCap = 2640;
constexpr int kStftAsmCap = 2640;

struct TwStride2 {                       // exp(-2 pi i t / H) out of the table of nFft = 2 H points
    const double2* __restrict__ w;
    __device__ __forceinline__ double2 operator()(int t, int /*nq*/) const { return w[2 * t]; }
};

__host__ __device__ inline int stft_pad(int F) { return F | 1; }   // an odd [bin] stride: no 2^k-way LDS bank conflicts

template <int NT>
__global__ __launch_bounds__(kStftThreads) void stft_kernel(const StftParams P, int F, int spanAlloc, long long runs) {
    extern __shared__ double2 stftLds[];
    constexpr int G = kStftThreads / NT;
    const int tid = threadIdx.x, g = tid / NT, t = tid % NT;
    const int N = P.nFft, H = N / 2, Fp = stft_pad(F);
    double2* const fftBuf = stftLds;                                  // [G][2][H]
    double* const span = (double*)(stftLds + 2 * G * H);              // [spanAlloc]
    double* const asmD = span + spanAlloc;                            // [(H + 1) Fp] ([2] under MRC_STFT_COMPLEX)
    double2* const asmC = (double2*)asmD;
    const long long blk = blockIdx.x, rc = blk / runs, run = blk - rc * runs, m0 = run * F;
    const int Fr = (int)(P.nFrames - m0 < F ? P.nFrames - m0 : F);
    const int hop = Fr > 1 ? (int)P.hop : 0;                          // (Fr > 1: the span fits the cap, so hop does)
    {
        const double* __restrict__ x = P.rows + rc * P.L + m0 * P.hop;
        const int len = (Fr - 1) * hop + N;                           // m0 hop + len <= L
        for (int i = tid; i < len; i += kStftThreads) span[i] = x[i];
    }
    __syncthreads();
    const TwStride2 W{P.tw};
    const bool complexOut = P.mode == MRC_STFT_COMPLEX;
    for (int f0 = 0; f0 < Fr; f0 += G) {
        const int f = f0 + g;
        const bool active = f < Fr;
        double2* A = fftBuf + 2 * g * H;
        double2* B = A + H;
        if (active) {
            const double* xs = span + f * hop;
            for (int n = t; n < H; n += NT)
                A[n] = make_double2(__dmul_rn(P.win[2 * n], xs[2 * n]), __dmul_rn(P.win[2 * n + 1], xs[2 * n + 1]));
        }
        __syncthreads();
        int p = 1;
        for (int s = 0; s < P.nRad; ++s) {
            const int R = (int)((P.radices >> (4 * s)) & 15);
            if (active) fft_pass_2345<TwStride2, NT>(R, A, B, H, p, W, t);
            __syncthreads();
            double2* sw = A; A = B; B = sw;
            p *= R;
        }
        if (active) {
            for (int k = t; k <= H; k += NT) {
                const double2 z = A[k == H ? 0 : k], y = A[k == 0 ? 0 : H - k];
                const double2 ev = make_double2(0.5 * (z.x + y.x), 0.5 * (z.y - y.y));
                const double2 od = make_double2(0.5 * (z.y + y.y), -0.5 * (z.x - y.x));
                const double2 r = cmul(P.tw[k], od);
                const double2 X = make_double2(ev.x + r.x, ev.y + r.y);
                if (complexOut) asmC[k * Fp + f] = X;
                else asmD[k * Fp + f] = __dadd_rn(__dmul_rn(X.x, X.x), __dmul_rn(X.y, X.y));
            }
        }
        __syncthreads();                                              // (the next round writes A; the assembly is read below)
    }
    int nOut = H + 1;
    const double* src = asmD;
    if (P.mode == MRC_STFT_BANK) {
        const int* __restrict__ lo = P.bankTab;
        const int* __restrict__ hi = lo + P.nFilters;
        const int* __restrict__ off = hi + P.nFilters;
        for (int idx = tid; idx < P.nFilters * Fr; idx += kStftThreads) {
            const int q = idx / Fr, f = idx - q * Fr, k0 = lo[q], k1 = hi[q];
            const double* __restrict__ w = P.bankW + off[q];
            double acc = 0.0;
            for (int k = k0; k < k1; ++k) acc = __dadd_rn(acc, __dmul_rn(w[k - k0], asmD[k * Fp + f]));
            span[q * Fp + f] = acc;
        }
        __syncthreads();
        nOut = P.nFilters;
        src = span;
    }
    const long long outBase = rc * nOut * P.nFrames + m0;
    for (int idx = tid; idx < nOut * Fr; idx += kStftThreads) {
        const int r = idx / Fr, f = idx - r * Fr;
        const long long o = outBase + (long long)r * P.nFrames + f;
        if (complexOut) {
            const double2 v = asmC[r * Fp + f];
            if (P.format == MRC_WINDOW_F64) ((double2*)P.out)[o] = v;
            else ((float2*)P.out)[o] = make_float2((float)v.x, (float)v.y);
        } else {
            const double v = src[r * Fp + f];
            if (P.format == MRC_WINDOW_F64) ((double*)P.out)[o] = v;
            else ((float*)P.out)[o] = (float)v;
        }
    }
}

}  // namespace

unsigned long long stft_radices(int n, int* nRad) {
    unsigned long long r = 0;
    int c = 0;
    for (int R : {4, 2, 3, 5})
        while (n % R == 0 && c < 16) {
            r |= (unsigned long long)R << (4 * c++);
            n /= R;
        }
    *nRad = c;
    return n == 1 ? r : 0;
}

// the frames a workgroup takes -- a function of the call's arguments alone -- its threads per transform and its LDS
struct StftPlan {
    int F, NT, spanAlloc;
    size_t lds;
};
StftPlan stft_plan(const StftParams& P) {
    const int N = P.nFft, H = N / 2, perBin = P.mode == MRC_STFT_COMPLEX ? 2 : 1;
    long long F = std::min<long long>(kStftMaxRun, P.nFrames);
    F = std::min<long long>(F, N >= kStftSpanCap ? 1 : (kStftSpanCap - N) / P.hop + 1);
    while (F > 1 && (long long)(H + 1) * stft_pad((int)F) * perBin > kStftAsmCap) --F;
    while (F > 1 && P.mode == MRC_STFT_BANK && (long long)P.nFilters * stft_pad((int)F) > kStftSpanCap) --F;
    F = std::max<long long>(F, 1);
    const int NT = N <= 512 ? 64 : N <= 1024 ? 128 : 256, G = kStftThreads / NT;
    if (F > G) F -= F % G;                                            // whole rounds of G transforms
    const int Fp = stft_pad((int)F);
    long long span = (F > 1 ? (F - 1) * P.hop : 0) + N;
    if (P.mode == MRC_STFT_BANK) span = std::max<long long>(span, (long long)P.nFilters * Fp);
    span += span & 1;                                                 // the assembly behind it holds double2
    const size_t lds = sizeof(double2) * 2 * (kStftThreads / NT) * H + sizeof(double) * (size_t)(span + (long long)(H + 1) * Fp * perBin);
    return StftPlan{(int)F, NT, (int)span, lds};
}

hipError_t launch_stft(const StftParams& P, hipStream_t st) {
    if (P.nRows <= 0 || P.nFrames <= 0) return hipSuccess;
    const StftPlan plan = stft_plan(P);
    const long long runs = (P.nFrames + plan.F - 1) / plan.F, units = (long long)P.nRows * P.nch;
    if (runs > 0x7fffffffLL / units) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(units * runs)), block(kStftThreads);
    auto go = [&](auto kernel) {
        hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, grid, block, plan.lds, st, P, plan.F, plan.spanAlloc, runs);
        return hipGetLastError();
    };
    if (plan.NT == 64) return go(stft_kernel<64>);
    if (plan.NT == 128) return go(stft_kernel<128>);
    return go(stft_kernel<256>);
}

}  // namespace mrc
