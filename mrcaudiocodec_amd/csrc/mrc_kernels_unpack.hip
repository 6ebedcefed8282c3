// `.pac` chunk parsing ON THE DEVICE: the decode half of the file layer (pacfileThem.py:176-302, 341-560) that
// mrc_unpack_blocks runs on host threads, with the parser of mrc_unpack.hpp -- the same source a host build of
// tests/unpack_check.cpp holds against mrc_unpack_blocks.
//
//   unpack_fixed_kernel   one lane per channel chunk, outputs in the fixed-stride layout of mrc_unpack_blocks
//                         (mrc_dev_unpack_blocks);
//   unpack_dense_kernel   one lane per channel chunk of a host plan, outputs straight into the dense per-(shape, kind)
//                         arrays decode_kernel reads, at the slot the plan gives (mrc_decode_pac_pcm16).  The plan lists
//                         the chunks of one (shape, kind, joint channel) together, so a wave's band loop has one trip
//                         count and only the escape branch of the Huffman decoding diverges;
//   pcm16_interleave_kernel  decoded planes -> WAV-order interleaved 16-bit codes per file (pcmfile.py:141-172), the
//                         first block of each file (the MDCT's half-block delay) dropped (pacfileThem.py:1176-1179).
//
// Every lane is a serial bit reader (at most ~1 000 codes per chunk); the decode tables (4 x 512 entries of
// value | length << 8) sit in LDS.  A chunk that does not parse sets a bit of its UnpackStatus in err->flag and
// lowers err->firstBad to its index; nothing it wrote is used (the host stops the call there).
#include "mrc_device.hpp"

namespace mrc {
using namespace dev;
namespace {

constexpr int kUnpackThreads = 256;

__device__ __forceinline__ void stage_tables(const UnpackTables* __restrict__ T, unsigned* sLut, int* sEsc) {
    const unsigned* src = (const unsigned*)T->lut;
    for (int i = threadIdx.x; i < kUnpackLutEntries / 2; i += blockDim.x) sLut[i] = src[i];
    if (threadIdx.x < 4) sEsc[threadIdx.x] = T->escape[threadIdx.x];
    __syncthreads();
}

__device__ __forceinline__ void report(UnpackErr* err, int64_t c, int rc) {
    atomicOr(&err->flag, 1 << rc);
    atomicMin(&err->firstBad, (int)(c < 0x7fffffff ? c : 0x7fffffff));
}

__global__ __launch_bounds__(kUnpackThreads) void unpack_fixed_kernel(UnpackParams P, UnpackBands B,
                                                                      const UnpackTables* __restrict__ T, int64_t nChunks,
                                                                      int nch, int joint, const uint8_t* __restrict__ buf,
                                                                      int64_t len, const int64_t* __restrict__ chunkOffset,
                                                                      UnpackFixedOut O, UnpackErr* err) {
    __shared__ unsigned sLut[kUnpackLutEntries / 2];
    __shared__ int sEsc[4];
    stage_tables(T, sLut, sEsc);
    const int64_t c = (int64_t)blockIdx.x * kUnpackThreads + threadIdx.x;
    if (c >= nChunks) return;
    const int rc = unpack_fixed_chunk(buf, len, chunkOffset, c / nch, (int)(c % nch), nch, joint, P, B,
                                      (const unsigned short*)sLut, sEsc, O);
    if (rc != kUnpackOk) report(err, c, rc);
}

__global__ __launch_bounds__(kUnpackThreads) void unpack_dense_kernel(UnpackParams P, UnpackBands B,
                                                                      const UnpackTables* __restrict__ T, int64_t nChunks,
                                                                      const UnpackPlanEntry* __restrict__ plan,
                                                                      const uint8_t* __restrict__ buf, int64_t len,
                                                                      const UnpackGroupDev* __restrict__ groups,
                                                                      UnpackErr* err) {
    __shared__ unsigned sLut[kUnpackLutEntries / 2];
    __shared__ int sEsc[4];
    stage_tables(T, sLut, sEsc);
    const int64_t c = (int64_t)blockIdx.x * kUnpackThreads + threadIdx.x;
    if (c >= nChunks) return;
    const UnpackPlanEntry e = plan[c];
    const int g = e.groupStream >> 1, stream = e.groupStream & 1;
    const UnpackGroupDev& G = groups[g];
    const int64_t slot = e.slot;
    const uint8_t* payload;
    int64_t nBytes;
    if (!unpack_locate(buf, len, e.off, &payload, &nBytes)) { report(err, c, kUnpackTruncated); return; }
    UnpackDst D;
    D.table = nullptr;
    if (G.joint) {
        D.oscale = stream == 0 ? G.oscale + slot * 4 : nullptr;
        D.ms = stream == 0 ? G.ms + slot * G.nb : nullptr;
        D.sf = G.sf + (slot * 2 + stream) * G.nb;
        D.ba = G.ba + (slot * 2 + stream) * G.nb;
        D.mant = G.mant + (slot * 2 + stream) * (int64_t)G.halfN;
    } else {
        D.oscale = G.oscale + slot;
        D.ms = nullptr;
        D.sf = G.sf + slot * G.nb;
        D.ba = G.ba + slot * G.nb;
        D.mant = G.mant + slot * (int64_t)G.halfN;
    }
    D.padBands = 0;
    D.padLines = 0;
    int shape;
    const int rc = unpack_chunk(payload, nBytes, P, B, (const unsigned short*)sLut, sEsc, G.joint, stream, G.shape, &shape, D);
    if (rc != kUnpackOk) report(err, c, rc);
}

// pcmfile.py:163-172 per value, as pcm16_kernel; the file of value i by binary search over outStart
__global__ void pcm16_interleave_kernel(int64_t nFiles, int64_t nOut, const long long* __restrict__ outStart,
                                        const long long* __restrict__ xStart, const int* __restrict__ nch, int skip,
                                        const double* __restrict__ x, int64_t planeStride, short* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nOut) return;
    int64_t lo = 0, hi = nFiles;                        // outStart[lo] <= i < outStart[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (outStart[mid] <= i) lo = mid; else hi = mid;
    }
    const int64_t local = i - outStart[lo];
    const int two = nch[lo] == 2;
    const int64_t t = two ? local >> 1 : local;
    const int c = two ? (int)(local & 1) : 0;
    const double v = x[c * planeStride + xStart[lo] + skip + t];
    const double mag = fabs(v);
    const int code = mag == 0.0 ? 0 : (int)mag_code(mag, 16);
    out[i] = (short)(signbit(v) ? -code : code);
}

}  // namespace

hipError_t launch_unpack_fixed(const UnpackParams& P, const UnpackBands& B, const UnpackTables* T, int64_t nBlocks, int nch,
                               int joint, const uint8_t* buf, int64_t len, const int64_t* chunkOffset, const UnpackFixedOut& O,
                               UnpackErr* err, hipStream_t st) {
    const int64_t n = nBlocks * nch;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(unpack_fixed_kernel, dim3((unsigned)((n + kUnpackThreads - 1) / kUnpackThreads)), dim3(kUnpackThreads),
                       0, st, P, B, T, n, nch, joint, buf, len, chunkOffset, O, err);
    return hipGetLastError();
}

hipError_t launch_unpack_dense(const UnpackParams& P, const UnpackBands& B, const UnpackTables* T, int64_t nChunks,
                               const UnpackPlanEntry* plan, const uint8_t* buf, int64_t len, const UnpackGroupDev* groups,
                               UnpackErr* err, hipStream_t st) {
    if (nChunks <= 0) return hipSuccess;
    hipLaunchKernelGGL(unpack_dense_kernel, dim3((unsigned)((nChunks + kUnpackThreads - 1) / kUnpackThreads)),
                       dim3(kUnpackThreads), 0, st, P, B, T, nChunks, plan, buf, len, groups, err);
    return hipGetLastError();
}

hipError_t launch_pcm16_interleave(int64_t nFiles, int64_t nOut, const long long* outStart, const long long* xStart,
                                   const int* nch, int skip, const double* x, int64_t planeStride, short* out,
                                   hipStream_t st) {
    if (nOut <= 0) return hipSuccess;
    hipLaunchKernelGGL(pcm16_interleave_kernel, dim3((unsigned)((nOut + 255) / 256)), dim3(256), 0, st, nFiles, nOut,
                       outStart, xStart, nch, skip, x, planeStride, out);
    return hipGetLastError();
}

}  // namespace mrc
