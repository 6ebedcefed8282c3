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
// Every sum that is compared with c or reported is nmr_band_kernel's: the mask terms pow(10, (T - 96) / 10) and the noise
// terms 4 (X - X^)^2 added in line order by one thread per band, the bands in band order by one thread per entry -- so the
// numbers are mrc_pac_nmr's of the file that is written, and max r <= c holds exactly wherever no band is capped.  No
// floating-point atomics.
#include "mrc_decode_lines.hpp"

namespace mrc {
using namespace dev;
namespace {

constexpr int kVbrThreads = 256;

__global__ __launch_bounds__(kVbrThreads) void vbr_alloc_kernel(
    DevShape S, int joint, int64_t n, int64_t k0, double ceiling, const double* __restrict__ phaseLines,
    const int* __restrict__ oscale, const int* __restrict__ msSwitch, int* __restrict__ bitAlloc,
    int* __restrict__ scaleFactor, unsigned short* __restrict__ mant, const long long* __restrict__ chunkMap,
    const double* __restrict__ lines, const double* __restrict__ thresh, double* __restrict__ stat,
    int* __restrict__ capped, long long chunkBase) {
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
                    if (cnt == 0 || (r[0] <= ceiling && r[1] <= ceiling)) sDone[j] = sDone[nb + j] = 1;
                    else {
                        double e0 = 0.0, e1 = 0.0;
                        for (int i = lo; i < lo + cnt; ++i) e0 += sErr[i];
                        for (int i = lo; i < lo + cnt; ++i) e1 += sErr[M + i];
                        int pick = e1 > e0 ? 1 : 0;       // the stream with the larger error; a tie: stream 0
                        if (sN[pick * nb + j] >= maxBits) pick ^= 1;
                        if (sN[pick * nb + j] >= maxBits) { sDone[j] = sDone[nb + j] = 1; sCap[j] = 1; }
                        else raise(pick * nb + j);
                    }
                }
            } else {
                for (int ch = 0; ch < ns; ++ch) {         // first fit per stream, against its own channel
                    const int t = ch * nb + j;
                    if (sDone[t]) continue;
                    if (cnt == 0 || r[ch] <= ceiling) sDone[t] = 1;
                    else if (sN[t] >= maxBits) { sDone[t] = 1; sCap[j] += 1; }
                    else raise(t);
                }
            }
        }
        if (!__syncthreads_or(more)) break;
    }

    const int nTot = ns * nb;
    if (tid < nTot) {
        bitAlloc[k * nTot + tid] = sN[tid];
        scaleFactor[k * nTot + tid] = sSf[tid];
    }
    for (int i = tid; i < ns * M; i += kVbrThreads) mant[k * ns * (int64_t)M + i] = sMant[i];
    if (tid < ns) {
        const int ch = tid;
        double mx = 0.0, sum = 0.0;
        int cap = 0;
        for (int j = 0; j < nb; ++j) {
            mx = fmax(mx, sR[ch * nb + j]);
            sum += sR[ch * nb + j];
            cap += sCap[j];
        }
        const long long chunk = chunkBase + chunkMap[kb * ns + ch];
        stat[2 * chunk] = mx;
        stat[2 * chunk + 1] = nb > 0 ? (double)S.b * (sum / (double)nb) : 0.0;
        capped[chunk] = ch == 0 ? cap : 0;                // a block's capped bands: counted at its first chunk
    }
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

}  // namespace mrc
