// Constant-quality VBR (mrc_encode_vbr_nmr_pac, mrc_api_chain.cpp; the rule: DESIGN.md section 12): every band gets the
// fewest mantissa bits that hold its MEASURED noise under a ceiling c relative to its mask.  No bit budget, no reservoir:
// a block depends on its own samples only.
//
//   vbr_alloc_kernel   one workgroup per block of one block-shape group (a joint block: both output channels, its M/S bands
//                      couple them).  LDS holds the quantiser's input (phase A's lines, scaled) per coded stream, a noise row
//                      per output channel, in joint blocks an error row per stream, and the candidate mantissas.  Every band
//                      carries a state -- n bits, or (n0, n1) in a joint block.  A pass quantises and decodes the lines of the
//                      unfinished bands at their state (mantissa_dev; decode_line, the code decode_kernel and nmr_band_kernel
//                      run, on the LDS-resident candidates), one thread per band sums its lines in line order, forms
//                      r = noise / mask and either finishes the band or raises its state (0 -> 2, else + 1).  At most 16
//                      passes without, 31 with M/S bands.  The last step writes the planes the device packer reads from the
//                      chained scan (bitAlloc, scaleFactor, uint16 mantissas) and the entry's {max_j r_j, b * mean_j r_j}
//                      for nmr_file_kernel.
//
//   vbr_profile_kernel the same walk with no ceiling (mrc_encode_vbr_size_pac): every band goes to the
//                      end of its state sequence and the ratio(s) of every state -- in an M/S band also the stream raised
//                      behind it -- are recorded.  The sequence is fixed by the signal; c only decides where it stops.
//   vbr_pick_kernel    the allocation for one ceiling per stream from that record: per band the first state whose test
//                      passes (the last one, capped, otherwise), ONE quantise pass at those states, and the planes, the
//                      entry statistics and the capped count exactly as vbr_alloc_kernel leaves them.
//   vbr_size_bytes_kernel  a stream's file size from the packer's plan: header + (4 + bytes) per chunk, in chunk order.
//
// Every sum that is compared with c or reported is nmr_band_kernel's: the mask terms pow(10, (T - 96) / 10) and the noise
// terms 4 (X - X^)^2 added in line order by one thread per band, the bands in band order by one thread per entry -- so the
// numbers are mrc_pac_nmr's of the file that is written, and max r <= c holds exactly wherever no band is capped.  No
// floating-point atomics.
#include "mrc_decode_lines.hpp"

namespace mrc {
using namespace dev;
namespace {

constexpr int kVbrThreads = 256;

// A block's record (vbr_profile_kernel -> vbr_pick_kernel): ratios [nBands][kVbrProfJoint or kVbrProfMono] and, in joint
// blocks, picks [nBands].  Non-joint band: r at state i (0, 2, 3, .. bits) in [i].  Joint L/R band: stream s's in
// [s * kVbrMsStates + i].  M/S band: {r_L, r_R} of step i in [2 i], [2 i + 1]; bit i of its pick word: the stream raised
// behind step i.
constexpr int kVbrMsStates = 31;                          // (0, 0) + 15 raises of either stream (maxMantBits <= 16)
constexpr int kVbrProfJoint = 2 * kVbrMsStates, kVbrProfMono = 16;

__device__ __forceinline__ int vbr_state_of_bits(int bits) { return bits ? bits - 1 : 0; }   // 0, 2, 3, .. -> 0, 1, 2, ..

// The entry statistics {max_j r_j, b * mean_j r_j} and a block's capped bands, bands in band order by one thread per entry
__device__ __forceinline__ void vbr_entry_stats(const DevShape& S, int nb, int ch, const double* sR, const int* sCap,
                                                long long chunk, double* __restrict__ stat, int* __restrict__ capped) {
    double mx = 0.0, sum = 0.0;
    int cap = 0;
    for (int j = 0; j < nb; ++j) {
        mx = fmax(mx, sR[ch * nb + j]);
        sum += sR[ch * nb + j];
        cap += sCap[j];
    }
    stat[2 * chunk] = mx;
    stat[2 * chunk + 1] = nb > 0 ? (double)S.b * (sum / (double)nb) : 0.0;
    capped[chunk] = ch == 0 ? cap : 0;                    // a block's capped bands: counted at its first chunk
}

// The walk of one block.  kProfile == false: vbr_alloc_kernel, a band stops at the first state that meets `ceiling`.
// kProfile == true: vbr_profile_kernel, no state stops a band that has lines; every state's ratios go to prof / profPick
// (this block's) and nothing else is written.
template <bool kProfile>
__device__ __forceinline__ void vbr_walk(
    const DevShape& S, int joint, int64_t n, int64_t k0, double ceiling, const double* __restrict__ phaseLines,
    const int* __restrict__ oscale, const int* __restrict__ msSwitch, int* __restrict__ bitAlloc,
    int* __restrict__ scaleFactor, unsigned short* __restrict__ mant, const long long* __restrict__ chunkMap,
    const double* __restrict__ lines, const double* __restrict__ thresh, double* __restrict__ stat,
    int* __restrict__ capped, long long chunkBase, double* __restrict__ prof, unsigned* __restrict__ profPick) {
    extern __shared__ double smem[];
    __shared__ double sMaskB[2 * kMaxBands], sR[2 * kMaxBands], sPeak[2 * kMaxBands];
    __shared__ int sN[2 * kMaxBands], sSf[2 * kMaxBands], sDone[2 * kMaxBands], sCap[kMaxBands], sMs[kMaxBands], sOs[4];
    const int tid = threadIdx.x;
    const int M = S.halfN, nb = S.nBands, nScaleBits = S.nScaleBits, maxBits = S.maxMantBits;
    const int ns = joint ? 2 : 1, nsig = joint ? 4 : 1;   // coded streams (= output channels), phase A's signals
    double* sNoise = smem;                                // [ns][M]: the mask terms first, then 4 (X - X^)^2 per output channel
    double* sQ = sNoise + ns * M;                         // [ns][M]: the quantiser's input per coded stream
    double* sErr = sQ + ns * M;                           // joint: [2][M] (x - x^)^2 of each stream, overall scale removed
    unsigned short* sMant = (unsigned short*)(sErr + (joint ? 2 * M : 0));   // [ns][M]: the candidates' codes
    const int64_t kb = blockIdx.x, k = k0 + kb;           // block of this launch / of the group
    const double* PL = phaseLines + k * nsig * (int64_t)M;
    const double* X[2] = {lines + kb * (int64_t)M, lines + (n + kb) * (int64_t)M};   // left rows, then right rows
    const double* T[2] = {thresh + kb * (int64_t)M, thresh + (n + kb) * (int64_t)M};

    if (tid < nsig) sOs[tid] = oscale[k * nsig + tid];
    if (tid < kMaxBands) {
        sMs[tid] = (joint && tid < nb) ? msSwitch[k * nb + tid] : 0;
        sCap[tid] = 0;
    }
    if (tid < 2 * kMaxBands) { sN[tid] = 0; sSf[tid] = 0; sDone[tid] = 0; sR[tid] = 0.0; }
    __syncthreads();
    for (int i = tid; i < M; i += kVbrThreads) {
        const int band = S.bandOfLine[i];
        for (int s = 0; s < ns; ++s) {
            const int sig = joint ? (sMs[band] == 1 ? 2 + s : s) : 0;         // stream 0: M or L, stream 1: S or R
            sQ[s * M + i] = ldexp(PL[sig * (int64_t)M + i], sOs[sig]);        // codecThem.py:323 (exact)
            sNoise[s * M + i] = pow(10.0, (T[s][i] - 96.0) / 10.0);           // psychoac.py:28-31 (Intensity)
        }
    }
    __syncthreads();
    if (tid < ns * nb) {                                  // (stream = channel s, band j): mask_j, max |scaled line|
        const int s = tid / nb, j = tid - s * nb;
        const int lo = S.bandLo[j], cnt = S.bandN[j];
        double mask = 0.0, peak = 0.0;
        for (int i = lo; i < lo + cnt; ++i) {
            mask += sNoise[s * M + i];
            peak = fmax(peak, fabs(sQ[s * M + i]));
        }
        sMaskB[tid] = mask;
        sPeak[tid] = peak;
        sSf[tid] = scale_factor_dev(peak, nScaleBits, 0);
    }
    __syncthreads();

    unsigned pickWord = 0;                                // kProfile, thread j: the streams its M/S band raised, a bit per step
    for (;;) {
        for (int i = tid; i < M; i += kVbrThreads) {
            const int band = S.bandOfLine[i];
            if (sDone[band] && (!joint || sDone[nb + band])) continue;
            for (int s = 0; s < ns; ++s) {
                const int bits = sN[s * nb + band];
                sMant[s * M + i] = bits ? (unsigned short)mantissa_dev(sQ[s * M + i], sSf[s * nb + band], nScaleBits, bits) : 0;
            }
            for (int ch = 0; ch < ns; ++ch) {
                const double xh = decode_line<unsigned short>(i, band, ch, joint != 0, nb, M, nScaleBits, sOs, sMs, sSf, sN, sMant);
                const double d = X[ch][i] - xh;
                sNoise[ch * M + i] = 4.0 * (d * d);       // psychoac.py:212: the line intensity 4 X^2 of the unscaled lines
            }
            if (joint && sMs[band] == 1)
                for (int s = 0; s < 2; ++s) {
                    const int bits = sN[s * nb + band];
                    const double xh = bits ? ldexp(dequantize_dev(sSf[s * nb + band], sMant[s * M + i], nScaleBits, bits), -sOs[2 + s]) : 0.0;
                    const double e = ldexp(sQ[s * M + i], -sOs[2 + s]) - xh;
                    sErr[s * M + i] = e * e;
                }
        }
        __syncthreads();
        int more = 0;
        if (tid < nb) {
            const int j = tid, lo = S.bandLo[j], cnt = S.bandN[j];
            const bool ms = joint && sMs[j] == 1;
            double* pj = kProfile ? prof + j * (joint ? kVbrProfJoint : kVbrProfMono) : nullptr;
            double r[2] = {0.0, 0.0};
            for (int ch = 0; ch < ns; ++ch) {
                if (sDone[ch * nb + j]) continue;
                double noise = 0.0;
                for (int i = lo; i < lo + cnt; ++i) noise += sNoise[ch * M + i];
                const double mask = sMaskB[ch * nb + j];
                r[ch] = isinf(mask) ? 0.0 : noise / mask;
                sR[ch * nb + j] = r[ch];
            }
            auto raise = [&](int t) {                     // 0 -> 2, else + 1; the band's scale factor follows its bits
                const int bits = sN[t] ? sN[t] + 1 : 2;
                sN[t] = bits;
                sSf[t] = scale_factor_dev(sPeak[t], nScaleBits, bits);
                more = 1;
            };
            if (ms) {
                if (!sDone[j]) {
                    [[maybe_unused]] const int step = vbr_state_of_bits(sN[j]) + vbr_state_of_bits(sN[nb + j]);
                    if constexpr (kProfile) { pj[2 * step] = r[0]; pj[2 * step + 1] = r[1]; }
                    if (cnt == 0 || (!kProfile && r[0] <= ceiling && r[1] <= ceiling)) sDone[j] = sDone[nb + j] = 1;
                    else {
                        double e0 = 0.0, e1 = 0.0;
                        for (int i = lo; i < lo + cnt; ++i) e0 += sErr[i];
                        for (int i = lo; i < lo + cnt; ++i) e1 += sErr[M + i];
                        int pick = e1 > e0 ? 1 : 0;       // the stream with the larger error; a tie: stream 0
                        if (sN[pick * nb + j] >= maxBits) pick ^= 1;
                        if (sN[pick * nb + j] >= maxBits) { sDone[j] = sDone[nb + j] = 1; sCap[j] = 1; }
                        else {
                            if constexpr (kProfile) pickWord |= (unsigned)pick << step;
                            raise(pick * nb + j);
                        }
                    }
                }
            } else {
                for (int ch = 0; ch < ns; ++ch) {         // first fit per stream, against its own channel
                    const int t = ch * nb + j;
                    if (sDone[t]) continue;
                    if constexpr (kProfile) pj[(joint ? ch * kVbrMsStates : 0) + vbr_state_of_bits(sN[t])] = r[ch];
                    if (cnt == 0 || (!kProfile && r[ch] <= ceiling)) sDone[t] = 1;
                    else if (sN[t] >= maxBits) { sDone[t] = 1; sCap[j] += 1; }
                    else raise(t);
                }
            }
        }
        if (!__syncthreads_or(more)) break;
    }

    if constexpr (kProfile) {
        if (joint && tid < nb) profPick[tid] = pickWord;
        return;
    }
    const int nTot = ns * nb;
    if (tid < nTot) {
        bitAlloc[k * nTot + tid] = sN[tid];
        scaleFactor[k * nTot + tid] = sSf[tid];
    }
    for (int i = tid; i < ns * M; i += kVbrThreads) mant[k * ns * (int64_t)M + i] = sMant[i];
    if (tid < ns) vbr_entry_stats(S, nb, tid, sR, sCap, chunkBase + chunkMap[kb * ns + tid], stat, capped);
}

__global__ __launch_bounds__(kVbrThreads) void vbr_alloc_kernel(
    DevShape S, int joint, int64_t n, int64_t k0, double ceiling, const double* __restrict__ phaseLines,
    const int* __restrict__ oscale, const int* __restrict__ msSwitch, int* __restrict__ bitAlloc,
    int* __restrict__ scaleFactor, unsigned short* __restrict__ mant, const long long* __restrict__ chunkMap,
    const double* __restrict__ lines, const double* __restrict__ thresh, double* __restrict__ stat,
    int* __restrict__ capped, long long chunkBase) {
    vbr_walk<false>(S, joint, n, k0, ceiling, phaseLines, oscale, msSwitch, bitAlloc, scaleFactor, mant, chunkMap, lines,
                    thresh, stat, capped, chunkBase, nullptr, nullptr);
}

// prof [blocks of the group][nBands][joint ? kVbrProfJoint : kVbrProfMono], profPick [blocks of the group][nBands] (joint)
__global__ __launch_bounds__(kVbrThreads) void vbr_profile_kernel(
    DevShape S, int joint, int64_t n, int64_t k0, const double* __restrict__ phaseLines, const int* __restrict__ oscale,
    const int* __restrict__ msSwitch, const double* __restrict__ lines, const double* __restrict__ thresh,
    double* __restrict__ prof, unsigned* __restrict__ profPick) {
    const int64_t k = k0 + blockIdx.x;
    vbr_walk<true>(S, joint, n, k0, 0.0, phaseLines, oscale, msSwitch, nullptr, nullptr, nullptr, nullptr, lines, thresh,
                   nullptr, nullptr, 0, prof + k * S.nBands * (joint ? kVbrProfJoint : kVbrProfMono),
                   joint ? profPick + k * S.nBands : nullptr);
}

// One workgroup per block k0 + kb of a group; ceilings [streams of the slab], chunkStream [chunks]: the stream of a chunk.
// LDS: the quantiser's input [ns][M].
__global__ __launch_bounds__(kVbrThreads) void vbr_pick_kernel(
    DevShape S, int joint, const double* __restrict__ ceilings, const int* __restrict__ chunkStream,
    const double* __restrict__ phaseLines, const int* __restrict__ oscale, const int* __restrict__ msSwitch,
    const double* __restrict__ prof, const unsigned* __restrict__ profPick, int* __restrict__ bitAlloc,
    int* __restrict__ scaleFactor, unsigned short* __restrict__ mant, const long long* __restrict__ chunkMap,
    double* __restrict__ stat, int* __restrict__ capped) {
    extern __shared__ double smem[];
    __shared__ double sR[2 * kMaxBands];
    __shared__ int sN[2 * kMaxBands], sSf[2 * kMaxBands], sCap[kMaxBands], sMs[kMaxBands], sOs[4];
    const int tid = threadIdx.x;
    const int M = S.halfN, nb = S.nBands, nScaleBits = S.nScaleBits, maxBits = S.maxMantBits;
    const int ns = joint ? 2 : 1, nsig = joint ? 4 : 1;
    double* sQ = smem;                                    // [ns][M]
    const int64_t k = blockIdx.x;
    const double* PL = phaseLines + k * nsig * (int64_t)M;
    const double ceiling = ceilings[chunkStream[chunkMap[k * ns]]];

    if (tid < nsig) sOs[tid] = oscale[k * nsig + tid];
    if (tid < kMaxBands) sMs[tid] = (joint && tid < nb) ? msSwitch[k * nb + tid] : 0;
    __syncthreads();
    for (int i = tid; i < M; i += kVbrThreads) {
        const int band = S.bandOfLine[i];
        for (int s = 0; s < ns; ++s) {
            const int sig = joint ? (sMs[band] == 1 ? 2 + s : s) : 0;
            sQ[s * M + i] = ldexp(PL[sig * (int64_t)M + i], sOs[sig]);
        }
    }
    if (tid < nb) {                                       // the walk of band j over its recorded states
        const int j = tid, cnt = S.bandN[j];
        const double* pj = prof + (k * nb + j) * (joint ? kVbrProfJoint : kVbrProfMono);
        int cap = 0;
        if (joint && sMs[j] == 1) {
            const unsigned picks = profPick[k * nb + j];
            int n0 = 0, n1 = 0, step = 0;
            double r0, r1;
            for (;;) {
                r0 = pj[2 * step]; r1 = pj[2 * step + 1];
                if (cnt == 0 || (r0 <= ceiling && r1 <= ceiling)) break;
                if (n0 >= maxBits && n1 >= maxBits) { cap = 1; break; }
                int pick = (picks >> step) & 1;           // (recorded behind the walk's own "the other one" rule)
                if ((pick ? n1 : n0) >= maxBits) pick ^= 1;
                if (pick) n1 = n1 ? n1 + 1 : 2;
                else n0 = n0 ? n0 + 1 : 2;
                ++step;
            }
            sN[j] = n0; sN[nb + j] = n1; sR[j] = r0; sR[nb + j] = r1;
        } else
            for (int ch = 0; ch < ns; ++ch) {
                const double* pc = pj + (joint ? ch * kVbrMsStates : 0);
                int bits = 0;
                double r;
                for (;;) {
                    r = pc[vbr_state_of_bits(bits)];
                    if (cnt == 0 || r <= ceiling) break;
                    if (bits >= maxBits) { cap += 1; break; }
                    bits = bits ? bits + 1 : 2;
                }
                sN[ch * nb + j] = bits; sR[ch * nb + j] = r;
            }
        sCap[j] = cap;
    }
    __syncthreads();
    const int nTot = ns * nb;
    if (tid < nTot) {                                     // the band's scale factor follows its bits
        const int j = tid % nb, s = tid / nb;
        const int lo = S.bandLo[j], cnt = S.bandN[j];
        double peak = 0.0;
        for (int i = lo; i < lo + cnt; ++i) peak = fmax(peak, fabs(sQ[s * M + i]));
        sSf[tid] = scale_factor_dev(peak, nScaleBits, sN[tid]);
        bitAlloc[k * nTot + tid] = sN[tid];
        scaleFactor[k * nTot + tid] = sSf[tid];
    }
    __syncthreads();
    for (int i = tid; i < ns * M; i += kVbrThreads) {
        const int s = i / M, t = s * nb + S.bandOfLine[i - s * M], bits = sN[t];
        mant[k * ns * (int64_t)M + i] = bits ? (unsigned short)mantissa_dev(sQ[i], sSf[t], nScaleBits, bits) : 0;
    }
    if (tid < ns) vbr_entry_stats(S, nb, tid, sR, sCap, chunkMap[k * ns + tid], stat, capped);
}

// bytes[s]: the file of stream s as the packer's plan prices it -- its header, and a 4-byte length in front of every chunk
__global__ void vbr_size_bytes_kernel(int64_t nStreams, int64_t nChunks, int hdrLen, const long long* __restrict__ firstChunk,
                                      const int* __restrict__ chunkBytes, long long* __restrict__ bytes) {
    const int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (s >= nStreams) return;
    const long long c1 = s + 1 < nStreams ? firstChunk[s + 1] : nChunks;
    long long sum = hdrLen;
    for (long long c = firstChunk[s]; c < c1; ++c) sum += 4 + chunkBytes[c];
    bytes[s] = sum;
}

}  // namespace

size_t vbr_lds_bytes(const DevShape& S, int joint) {
    const size_t M = (size_t)S.halfN;
    return joint ? 6 * M * sizeof(double) + 2 * M * sizeof(unsigned short) : 2 * M * sizeof(double) + M * sizeof(unsigned short);
}

hipError_t launch_vbr_alloc(const DevShape& S, int joint, int64_t n, int64_t k0, double ceiling, const double* phaseLines,
                            const int* oscale, const int* msSwitch, int* bitAlloc, int* scaleFactor, unsigned short* mant,
                            const long long* chunkMap, const double* lines, const double* thresh, double* stat, int* capped,
                            long long chunkBase, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (S.nBands > kMaxBands || vbr_lds_bytes(S, joint) > 60 * 1024) return hipErrorInvalidValue;   // (chain_shape_misfit holds)
    hipLaunchKernelGGL(vbr_alloc_kernel, dim3((unsigned)n), dim3(kVbrThreads), vbr_lds_bytes(S, joint), st, S, joint, n, k0,
                       ceiling, phaseLines, oscale, msSwitch, bitAlloc, scaleFactor, mant, chunkMap, lines, thresh, stat,
                       capped, chunkBase);
    return hipGetLastError();
}

size_t vbr_profile_bytes(const DevShape& S, int joint) {
    return (size_t)S.nBands * (joint ? kVbrProfJoint : kVbrProfMono) * sizeof(double);
}

hipError_t launch_vbr_profile(const DevShape& S, int joint, int64_t n, int64_t k0, const double* phaseLines, const int* oscale,
                              const int* msSwitch, const double* lines, const double* thresh, double* prof, unsigned* profPick,
                              hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (S.nBands > kMaxBands || S.maxMantBits > kVbrProfMono || vbr_lds_bytes(S, joint) > 60 * 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vbr_profile_kernel, dim3((unsigned)n), dim3(kVbrThreads), vbr_lds_bytes(S, joint), st, S, joint, n, k0,
                       phaseLines, oscale, msSwitch, lines, thresh, prof, profPick);
    return hipGetLastError();
}

hipError_t launch_vbr_pick(const DevShape& S, int joint, int64_t n, const double* ceilings, const int* chunkStream,
                           const double* phaseLines, const int* oscale, const int* msSwitch, const double* prof,
                           const unsigned* profPick, int* bitAlloc, int* scaleFactor, unsigned short* mant,
                           const long long* chunkMap, double* stat, int* capped, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (S.nBands > kMaxBands || S.maxMantBits > kVbrProfMono) return hipErrorInvalidValue;
    const size_t lds = (size_t)(joint ? 2 : 1) * S.halfN * sizeof(double);
    hipLaunchKernelGGL(vbr_pick_kernel, dim3((unsigned)n), dim3(kVbrThreads), lds, st, S, joint, ceilings, chunkStream,
                       phaseLines, oscale, msSwitch, prof, profPick, bitAlloc, scaleFactor, mant, chunkMap, stat, capped);
    return hipGetLastError();
}

hipError_t launch_vbr_size_bytes(int64_t nStreams, int64_t nChunks, int hdrLen, const long long* firstChunk,
                                 const int* chunkBytes, long long* bytes, hipStream_t st) {
    if (nStreams <= 0) return hipSuccess;
    hipLaunchKernelGGL(vbr_size_bytes_kernel, dim3((unsigned)((nStreams + 255) / 256)), dim3(256), 0, st, nStreams, nChunks,
                       hdrLen, firstChunk, chunkBytes, bytes);
    return hipGetLastError();
}

}  // namespace mrc
