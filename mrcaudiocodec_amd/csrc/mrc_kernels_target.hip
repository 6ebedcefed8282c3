// Encode to a target noise-to-mask ratio (mrc_encode_chained_target_nmr_pac, mrc_api_chain.cpp): the NMR of every rung of a
// chained rate ladder, computed from the serial scan's own planes while they are in device memory, and the gather of the
// chosen files.
//
//   nmr_rungs_kernel      one workgroup per entry (block, output channel) of one block-shape group.  The mask terms
//                         10^((T - 96) / 10) of the entry's lines go into LDS ONCE and every band's mask_j is summed once;
//                         then, rung after rung, the decoded lines of the rung's planes (decode_line, the code decode_kernel
//                         and nmr_band_kernel run) give 4 (X - X^)^2 in the second LDS row, one thread per band sums its
//                         lines in line order, thread 0 sums the bands in band order:
//                         stat[rung][entry] = {max_j r_j, b * mean_j r_j}.  The arithmetic and the order of every sum are
//                         nmr_band_kernel's (mrc_kernels_nmr.hip), so the numbers are mrc_pac_nmr's of the rung's file;
//                         what the rungs share -- one pow per line -- is paid once.
//   target_gather_kernel  the chosen file of every stream, from the rungs' packed bytes to one contiguous run in stream order.
//
// The file reduction is nmr_file_kernel (launch_nmr_file) over [rungs x streams] pseudo-files.  No floating-point atomics.
#include "mrc_decode_lines.hpp"

#include <algorithm>

namespace mrc {
using namespace dev;
namespace {

constexpr int kRungThreads = 256;

__global__ __launch_bounds__(kRungThreads) void nmr_rungs_kernel(DevShape S, int nRates, int joint, int64_t n, int64_t k0,
                                                                const ChainGroupDev* __restrict__ groups, int g,
                                                                const long long* __restrict__ chunkMap,
                                                                const double* __restrict__ lines,
                                                                const double* __restrict__ thresh,
                                                                double* __restrict__ stat, long long statStride,
                                                                long long chunkBase) {
    extern __shared__ double smem[];
    __shared__ double sR[kMaxBands];
    const int tid = threadIdx.x;
    const int M = S.halfN, nb = S.nBands;
    double* sMask = smem;                               // [M]
    double* sNoise = smem + M;                          // [M]
    const int nOut = joint ? 2 : 1;
    const int64_t e = blockIdx.x;                       // entry of this launch: (block k0 + kb, output channel ch)
    const int64_t kb = e / nOut;
    const int ch = (int)(e - kb * nOut);
    const int64_t k = k0 + kb;                          // block of the group
    const int64_t row = joint ? ch * n + kb : kb;       // the source analysis: left rows, then right rows
    const double* X = lines + row * M;
    const double* T = thresh + row * M;
    const long long chunk = chunkBase + chunkMap[e];    // the entry's place in its stream's file order

    for (int i = tid; i < M; i += kRungThreads) sMask[i] = pow(10.0, (T[i] - 96.0) / 10.0);   // psychoac.py:28-31 (Intensity)
    __syncthreads();
    double mask = 0.0;
    int lo = 0, cnt = 0;
    if (tid < nb) {
        lo = S.bandLo[tid];
        cnt = S.bandN[tid];
        for (int i = lo; i < lo + cnt; ++i) mask += sMask[i];
    }
    for (int r = 0; r < nRates; ++r) {
        const ChainGroupDev& D = groups[r * kChainGroups + g];
        const int* os = D.oscale + k * (joint ? 4 : 1);
        const int* ms = joint ? D.ms + k * nb : nullptr;
        const int* sf = D.scaleFactor + k * D.nTot;
        const int* ba = D.bitAlloc + k * D.nTot;
        const unsigned short* mant = D.mant + k * D.nstream * (int64_t)M;
        for (int i = tid; i < M; i += kRungThreads) {
            const double xh = decode_line(i, S.bandOfLine[i], ch, joint != 0, nb, M, S.nScaleBits, os, ms, sf, ba, mant);
            const double d = X[i] - xh;
            sNoise[i] = 4.0 * (d * d);                  // psychoac.py:212: the line intensity 4 X^2 of the unscaled lines
        }
        __syncthreads();
        if (tid < nb) {
            double noise = 0.0;
            for (int i = lo; i < lo + cnt; ++i) noise += sNoise[i];
            sR[tid] = isinf(mask) ? 0.0 : noise / mask;
        }
        __syncthreads();
        if (tid == 0) {
            double mx = 0.0, sum = 0.0;
            for (int j = 0; j < nb; ++j) {
                mx = fmax(mx, sR[j]);
                sum += sR[j];
            }
            double* out = stat + 2 * (r * statStride + chunk);
            out[0] = mx;
            out[1] = nb > 0 ? (double)S.b * (sum / (double)nb) : 0.0;
        }
        // (the next rung's lines overwrite sNoise only behind the barrier the band sums finished in front of, and its band
        //  ratios overwrite sR only behind the barrier thread 0 reaches after reading them)
    }
}

__global__ __launch_bounds__(256) void target_gather_kernel(int64_t nStreams, const long long* __restrict__ span,
                                                           const unsigned char* __restrict__ in,
                                                           unsigned char* __restrict__ out) {
    for (int64_t s = blockIdx.y; s < nStreams; s += gridDim.y) {
        const long long src = span[3 * s], dst = span[3 * s + 1], len = span[3 * s + 2];
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < len; i += (long long)gridDim.x * 256)
            out[dst + i] = in[src + i];
    }
}

}  // namespace

hipError_t launch_nmr_rungs(const DevShape& S, int nRates, int joint, int64_t n, int64_t k0, const ChainGroupDev* groups,
                            int g, const long long* chunkMap, const double* lines, const double* thresh, double* stat,
                            long long statStride, long long chunkBase, hipStream_t st) {
    if (n <= 0 || nRates <= 0) return hipSuccess;
    const size_t lds = sizeof(double) * 2 * (size_t)S.halfN;
    hipLaunchKernelGGL(nmr_rungs_kernel, dim3((unsigned)(n * (joint ? 2 : 1))), dim3(kRungThreads), lds, st, S, nRates, joint, n,
                       k0, groups, g, chunkMap, lines, thresh, stat, statStride, chunkBase);
    return hipGetLastError();
}

hipError_t launch_target_gather(int64_t nStreams, int64_t maxLen, const long long* span, const unsigned char* in,
                                unsigned char* out, hipStream_t st) {
    if (nStreams <= 0 || maxLen <= 0) return hipSuccess;
    const unsigned gx = (unsigned)std::min<int64_t>((maxLen + 255) / 256, 2048);
    const unsigned gy = (unsigned)std::min<int64_t>(nStreams, 65535);
    hipLaunchKernelGGL(target_gather_kernel, dim3(gx, gy), dim3(256), 0, st, nStreams, span, in, out);
    return hipGetLastError();
}

}  // namespace mrc
