// Noise-to-mask ratio of decoded `.pac` blocks against the source they were coded from (mrc_pac_nmr, mrc_api_nmr.cpp).
//
//   nmr_pad_kernel    the caller's int16 samples -> padded source planes: n_mdct_lines zeros, the samples, zeros to the
//                     plane's length (the stream with its prior hop that the chained encoder reads)
//   nmr_band_kernel   one workgroup per entry (block, channel): the decoded lines X^ of the channel (decode_line, the
//                     code decode_kernel runs), the source's MDCT lines X and masked threshold T (launch_mdct and
//                     launch_smr, unchanged) -> per band  noise_j = sum 4 (X - X^)^2,  mask_j = sum 10^((T - 96) / 10),
//                     r_j = noise_j / mask_j (0 where mask_j is +inf); per entry max_j r_j and b * mean_j r_j
//   nmr_file_kernel   one workgroup per file: its entries -> max r, sum of b * mean r, blocks with some r_j > 1
//
// Determinism: every sum has one fixed order.  A band's lines are added one after the other by one thread, its bands by
// one thread, and a file's entries in 256 fixed contiguous runs followed by a fixed tree.  Nothing depends on how many
// files or entries a call holds, on the order in which workgroups run, or on the deduplication of the source analysis
// (a shared analysis is the same bits as a repeated one).  No floating-point atomics.
//
// 10^x: pow(10.0, x) of the HIP math library (double precision, at most 1 ulp of error by its documentation), the
// function smr_kernel's exact spreading mode calls for the same quantity.
#include "mrc_decode_lines.hpp"

namespace mrc {
using namespace dev;
namespace {

constexpr int kNmrThreads = 256;

__global__ __launch_bounds__(kNmrThreads) void nmr_pad_kernel(int64_t nPlanes, const NmrPlane* __restrict__ planes, int L,
                                                             const short* __restrict__ src, short* __restrict__ out) {
    for (int64_t p = blockIdx.y; p < nPlanes; p += gridDim.y) {
        const NmrPlane P = planes[p];
        for (int64_t t = (int64_t)blockIdx.x * kNmrThreads + threadIdx.x; t < P.len; t += (int64_t)gridDim.x * kNmrThreads) {
            const int64_t u = t - L;
            out[P.dst + t] = (u >= 0 && u < P.frames) ? src[P.src + u] : (short)0;
        }
    }
}

__global__ __launch_bounds__(kNmrThreads) void nmr_band_kernel(DevShape S, const NmrEntry* __restrict__ entries,
                                                              const UnpackGroupDev* __restrict__ groups,
                                                              const double* __restrict__ lines,
                                                              const double* __restrict__ thresh,
                                                              double* __restrict__ bandNoise, double* __restrict__ bandMask,
                                                              double* __restrict__ stat) {
    extern __shared__ double smem[];
    __shared__ double sR[kMaxBands];
    const int tid = threadIdx.x;
    const int M = S.halfN, nb = S.nBands;
    double* sNoise = smem;                              // [M]
    double* sMask = smem + M;                           // [M]
    const NmrEntry e = entries[blockIdx.x];
    const UnpackGroupDev& G = groups[e.group];
    const bool joint = G.joint != 0;
    const int ns = joint ? 2 : 1;
    const int64_t slot = e.slot;
    const int* os = G.oscale + slot * (joint ? 4 : 1);
    const int* ms = joint ? G.ms + slot * nb : nullptr;
    const int* sf = G.sf + slot * ns * nb;
    const int* ba = G.ba + slot * ns * nb;
    const int* mant = G.mant + slot * ns * (int64_t)M;
    const double* X = lines + e.ana * M;
    const double* T = thresh + e.ana * M;

    for (int k = tid; k < M; k += kNmrThreads) {
        const double xh = decode_line(k, S.bandOfLine[k], e.ch, joint, nb, M, S.nScaleBits, os, ms, sf, ba, mant);
        const double d = X[k] - xh;
        sNoise[k] = 4.0 * (d * d);                      // psychoac.py:212: the line intensity 4 X^2 of the unscaled lines
        sMask[k] = pow(10.0, (T[k] - 96.0) / 10.0);     // psychoac.py:28-31 (Intensity)
    }
    __syncthreads();
    if (tid < kMaxBands) {
        double noise = 0.0, mask = 0.0, r = 0.0;
        if (tid < nb) {
            const int lo = S.bandLo[tid], n = S.bandN[tid];
            for (int k = lo; k < lo + n; ++k) {
                noise += sNoise[k];
                mask += sMask[k];
            }
            r = isinf(mask) ? 0.0 : noise / mask;
            sR[tid] = r;
        }
        if (bandNoise) {
            bandNoise[e.out * kMaxBands + tid] = noise;
            bandMask[e.out * kMaxBands + tid] = mask;
        }
    }
    __syncthreads();
    if (tid == 0) {
        double mx = 0.0, sum = 0.0;
        for (int j = 0; j < nb; ++j) {
            mx = fmax(mx, sR[j]);
            sum += sR[j];
        }
        stat[2 * e.out] = mx;
        stat[2 * e.out + 1] = nb > 0 ? (double)e.b * (sum / (double)nb) : 0.0;
    }
}

__global__ __launch_bounds__(kNmrThreads) void nmr_file_kernel(const long long* __restrict__ entryStart,
                                                              const int* __restrict__ nch, const double* __restrict__ stat,
                                                              double* __restrict__ fileOut) {
    __shared__ double sMax[kNmrThreads], sSum[kNmrThreads];
    __shared__ long long sCnt[kNmrThreads];
    const int tid = threadIdx.x;
    const int64_t f = blockIdx.x;
    const int64_t e0 = entryStart[f], c = nch[f];
    const int64_t nBlk = (entryStart[f + 1] - e0) / c;
    // thread t: blocks [nBlk t / T, nBlk (t + 1) / T), entries in order
    const int64_t b0 = nBlk * tid / kNmrThreads, b1 = nBlk * (tid + 1) / kNmrThreads;
    double mx = 0.0, sum = 0.0;
    long long cnt = 0;
    for (int64_t i = b0; i < b1; ++i) {
        bool disturbed = false;
        for (int64_t ch = 0; ch < c; ++ch) {
            const int64_t e = e0 + i * c + ch;
            const double m = stat[2 * e];
            mx = fmax(mx, m);
            sum += stat[2 * e + 1];
            disturbed |= m > 1.0;
        }
        cnt += disturbed ? 1 : 0;
    }
    sMax[tid] = mx;
    sSum[tid] = sum;
    sCnt[tid] = cnt;
    __syncthreads();
    for (int w = kNmrThreads / 2; w > 0; w >>= 1) {
        if (tid < w) {
            sMax[tid] = fmax(sMax[tid], sMax[tid + w]);
            sSum[tid] = sSum[tid] + sSum[tid + w];
            sCnt[tid] += sCnt[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        fileOut[4 * f] = sMax[0];
        fileOut[4 * f + 1] = sSum[0];
        fileOut[4 * f + 2] = (double)sCnt[0];
        fileOut[4 * f + 3] = 0.0;
    }
}

}  // namespace

hipError_t launch_nmr_pad(int64_t nPlanes, const NmrPlane* planes, int64_t maxLen, int L, const short* src, short* out,
                          hipStream_t st) {
    if (nPlanes <= 0 || maxLen <= 0) return hipSuccess;
    const unsigned gx = (unsigned)std::min<int64_t>((maxLen + kNmrThreads - 1) / kNmrThreads, 4096);
    const unsigned gy = (unsigned)std::min<int64_t>(nPlanes, 65535);
    hipLaunchKernelGGL(nmr_pad_kernel, dim3(gx, gy), dim3(kNmrThreads), 0, st, nPlanes, planes, L, src, out);
    return hipGetLastError();
}

hipError_t launch_nmr_band(const DevShape& S, int64_t nEntries, const NmrEntry* entries, const UnpackGroupDev* groups,
                           const double* lines, const double* thresh, double* bandNoise, double* bandMask, double* stat,
                           hipStream_t st) {
    if (nEntries <= 0) return hipSuccess;
    const size_t lds = sizeof(double) * 2 * (size_t)S.halfN;
    hipLaunchKernelGGL(nmr_band_kernel, dim3((unsigned)nEntries), dim3(kNmrThreads), lds, st, S, entries, groups, lines,
                       thresh, bandNoise, bandMask, stat);
    return hipGetLastError();
}

hipError_t launch_nmr_file(int64_t nFiles, const long long* entryStart, const int* nch, const double* stat, double* fileOut,
                           hipStream_t st) {
    if (nFiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(nmr_file_kernel, dim3((unsigned)nFiles), dim3(kNmrThreads), 0, st, entryStart, nch, stat, fileOut);
    return hipGetLastError();
}

}  // namespace mrc
