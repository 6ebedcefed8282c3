// Decode side on gfx950 ("next" row f-4): codecThem.py:30-134 (Decode / JointDecode) with the overlap-and-add of
// pacfileThem.py:312-315 fused, and the 16-bit PCM codes of pcmfile.py:163-172.
//
//   decode_kernel   one workgroup per (block, output channel), any block shape:
//     vDequantize (quantize.py:325-357, operation order kept: ((sign*mag)*2) / (2^R - 1), one correctly rounded
//     division) -> divide by the overall scale level (a power of two: exact) -> ReconstructLR (ms_stereo.py:33-49;
//     a joint block's output channel dequantises BOTH streams of the bands whose M/S switch is set)
//     -> IMDCT (mdct.py:98-122) as a DCT-IV through the same N/4-point complex FFT, twiddles and signed circular
//     shift as the forward kernel (the transform matrix is the transpose of the forward one, so the fold becomes
//     an unfold) -> transition window (window.py:104-121) -> atomic add into the output stream at the block's
//     offset.  Every output sample receives at most two contributions and a + b == b + a, so the result does not
//     depend on the order in which blocks finish.
//   decode_mix_kernel, decode_reduced_mix_kernel   one workgroup per block into ONE plane: its left or right channel, or
//     the mid (L + R) / 2 formed on the lines before the one inverse transform (decode_line_mid; the store's mix windows).
//   decode_reduced_kernel   the same block at 1 / D of its sample rate: its first halfN / D lines through the inverse
//     transform of the shape (a, b) / D (the resident store's reduced windows, mrc_api_store.cpp).
//   decode_shaped_kernel, decode_shaped_mix_kernel, decode_reduced_shaped_kernel, decode_reduced_shaped_mix_kernel   the four
//     store launches above with one band gain per line between the dequantiser and the inverse transform
//     (mrc_pac_store_decode_window_shaped): decode_block<.., true>, the unshaped instantiations keep their code.
//   pcm16_kernel    |x| -> 16-bit magnitude code (quantize.py:61-87) with the sign re-applied as 2's complement.
//
// The reference computes the IMDCT with an N-point complex inverse FFT; like the forward transform the results
// agree to ~1e-13 of the block's peak (tests hold 1e-12).
#include "mrc_decode_lines.hpp"

namespace mrc {
using namespace dev;
namespace {

// One block into one output plane.  S: the shape whose transform, window and LDS layout are used; the parsed arrays are those
// of a block of nb bands and lineStride lines per stream with the band table bandOfLine, of which the first S.halfN lines
// are dequantised.  decode_kernel: all of them S's own.  decode_reduced_kernel: the block's full shape, S its reduced one.
// f: the block's slot in the parsed arrays (joint: two streams per slot, else one).  sel: what the plane receives --
// 0 / 1: output channel L / R (a non-joint slot has one channel: itself); kSelMid: (L + R) / 2 on the lines, which for a
// non-joint slot means the PAIR of slots f, f + 1, a stereo file's last block (its two chunks side by side are laid out
// as one slot of two streams, each with its own overall scale).  out: the plane, at the block's first sample.
// kMix false: sel is a channel, and the two-plane kernels hold no code for the mid.
// kShaped (mrc_pac_store_decode_window_shaped): line k, as the unshaped block transforms it, is multiplied once by
// gainRow[lineBand[k]] -- lineBand the uint16 band of every line of the block's FULL shape (coalesced), kNoLineBand where the
// line lies in no band and is left as it is; gainRow the unit's row of band gains (at most 2 KB, read by every lane of the
// workgroup: it stays in cache).  No LDS beyond the unshaped block's.
constexpr int kSelMid = 2;
template <bool kShaped>
__device__ __forceinline__ double shape_line(double x, int k, const unsigned short* __restrict__ lineBand,
                                             const double* __restrict__ gainRow) {
    if (kShaped) {
        const unsigned short q = lineBand[k];
        if (q != kNoLineBand) x = __dmul_rn(gainRow[q], x);
    }
    return x;
}
template <bool kMix, bool kShaped = false>
__device__ __forceinline__ void decode_block(const DevShape& S, const unsigned char* __restrict__ bandOfLine, int nb,
                                             int lineStride, int nScaleBits, bool joint, int64_t f, int sel,
                                             const int* __restrict__ oscale, const int* __restrict__ msSwitch,
                                             const int* __restrict__ scaleFactor, const int* __restrict__ bitAlloc,
                                             const int* __restrict__ mantissa, double* __restrict__ out, double* smem,
                                             const unsigned short* __restrict__ lineBand = nullptr,
                                             const double* __restrict__ gainRow = nullptr) {
    const int tid = threadIdx.x;
    const int N = S.N, M = S.halfN, Q = S.Q;
    const int nStreams = joint ? 2 : 1;
    double* v = smem;                                   // [M] lines, later the DCT-IV output; [M, N) unused
    double2* A = (double2*)(smem + N);                  // [Q]
    double2* B = A + Q;                                 // [Q]
    const int* sf = scaleFactor + f * nStreams * nb;
    const int* ba = bitAlloc + f * nStreams * nb;
    const int* mant = mantissa + f * nStreams * (int64_t)lineStride;
    const int* os = oscale + f * (joint ? 4 : 1);
    const int* ms = joint ? msSwitch + f * nb : nullptr;

    // dequantise, undo the overall scale (codecThem.py:47-51, 92-109), rebuild L / R (ms_stereo.py:33-49) or the mid
    if (!kMix || sel != kSelMid) {
        for (int k = tid; k < M; k += kThreads)
            v[k] = shape_line<kShaped>(decode_line(k, bandOfLine[k], sel, joint, nb, lineStride, nScaleBits, os, ms, sf, ba, mant), k,
                                       lineBand, gainRow);
    } else if (joint) {
        for (int k = tid; k < M; k += kThreads)
            v[k] = shape_line<kShaped>(decode_line_mid(k, bandOfLine[k], nb, lineStride, nScaleBits, os, ms, sf, ba, mant), k, lineBand,
                                       gainRow);
    } else {
        for (int k = tid; k < M; k += kThreads) {
            const int band = bandOfLine[k];
            const double x0 = decode_line(k, band, 0, false, nb, lineStride, nScaleBits, os, nullptr, sf, ba, mant);
            const double x1 = decode_line(k, band, 0, false, nb, lineStride, nScaleBits, os + 1, nullptr, sf + nb, ba + nb,
                                          mant + lineStride);
            v[k] = shape_line<kShaped>(0.5 * (x0 + x1), k, lineBand, gainRow);
        }
    }
    __syncthreads();
    // DCT-IV of the lines through the N/4-point FFT (same pairing and twiddles as the forward kernel)
    for (int n = tid; n < Q; n += kThreads) A[n] = cmul(make_double2(v[2 * n], v[M - 1 - 2 * n]), S.pre[n]);
    __syncthreads();
    double2* T = fft_lds(A, B, Q, S.radQ, S.nRadQ, S.wQ, tid);
    for (int k = tid; k < Q; k += kThreads) {
        const double2 c = cmul(T[k], S.post[k]);
        v[2 * k] = c.x;
        v[M - 1 - 2 * k] = -c.y;
    }
    __syncthreads();
    // unfold M -> N (transpose of the forward fold), undo the signed circular shift, x = 2 y (mdct.py:121 scales by N
    // what its normalised inverse FFT divided by N; the remaining factor is the 2 of the definition), window, add
    const int h = Q;
    for (int i = tid; i < N; i += kThreads) {
        int m = i + S.shift;
        double sgn = 2.0;
        if (m < 0) { m += N; sgn = -2.0; }
        else if (m >= N) { m -= N; sgn = -2.0; }
        double y;
        if (m < h) y = v[h + m];
        else if (m < 2 * h) y = -v[3 * h - 1 - m];
        else if (m < 3 * h) y = -v[3 * h - 1 - m];
        else y = -v[m - 3 * h];
        unsafeAtomicAdd(out + i, (sgn * y) * S.win[i]);
    }
}

// workgroup -> (block, output channel) of the two-plane launches: one workgroup per stream of every slot
struct BlockChannel { int64_t f; int ch; };
__device__ __forceinline__ BlockChannel block_channel(int nStreams) {
    return BlockChannel{(int64_t)(blockIdx.x / nStreams), (int)(blockIdx.x % nStreams)};
}
// workgroup w -> slot of the one-plane (mix) launches.  Joint group: slot w.  Non-joint group: its first 2 nPairs slots are
// the pairs (workgroup w < nPairs: slots 2 w, 2 w + 1, their mid), the rest single slots (a mono file's block, or the one
// parsed channel of a stereo file's last block).  outOffset is indexed by the workgroup.
__device__ __forceinline__ void mix_slot(bool joint, int mixSel, int64_t nPairs, int64_t* f, int* sel) {
    const int64_t w = blockIdx.x;
    if (joint) { *f = w; *sel = mixSel; }
    else if (w < nPairs) { *f = 2 * w; *sel = kSelMid; }
    else { *f = w + nPairs; *sel = 0; }
}

__global__ __launch_bounds__(kThreads) void decode_kernel(DevShape S, int nStreams, const int* __restrict__ oscale,
                                                          const int* __restrict__ msSwitch,
                                                          const int* __restrict__ scaleFactor,
                                                          const int* __restrict__ bitAlloc,
                                                          const int* __restrict__ mantissa,
                                                          const int64_t* __restrict__ outOffset,
                                                          double* __restrict__ outL, double* __restrict__ outR) {
    extern __shared__ double smem[];
    const BlockChannel bc = block_channel(nStreams);
    decode_block<false>(S, S.bandOfLine, S.nBands, S.halfN, S.nScaleBits, nStreams == 2, bc.f, bc.ch, oscale, msSwitch, scaleFactor,
                 bitAlloc, mantissa, (bc.ch == 0 ? outL : outR) + outOffset[bc.f], smem);
}

// ... one plane per item (the store's mix windows): one workgroup per joint slot, pair or single slot (mix_slot)
__global__ __launch_bounds__(kThreads) void decode_mix_kernel(DevShape S, int joint, int mixSel, int64_t nPairs,
                                                              const int* __restrict__ oscale,
                                                              const int* __restrict__ msSwitch,
                                                              const int* __restrict__ scaleFactor,
                                                              const int* __restrict__ bitAlloc,
                                                              const int* __restrict__ mantissa,
                                                              const int64_t* __restrict__ outOffset,
                                                              double* __restrict__ out) {
    extern __shared__ double smem[];
    int64_t f;
    int sel;
    mix_slot(joint != 0, mixSel, nPairs, &f, &sel);
    decode_block<true>(S, S.bandOfLine, S.nBands, S.halfN, S.nScaleBits, joint != 0, f, sel, oscale, msSwitch, scaleFactor, bitAlloc,
                 mantissa, out + outOffset[blockIdx.x], smem);
}

// The block at 1 / D of its sample rate (the store's reduced windows): the first R.halfN = halfN / D of its lines through
// the inverse transform of the shape R = (a, b) / D.  With n = D m + (D - 1) / 2 the phase (n + n0)(k + 1/2) / N of the
// full block's line k at sample n is (m + n0')(k + 1/2) / N' of R's line k at sample m, and the inverse carries no factor
// that depends on N: the result is the block's signal band-limited to the new Nyquist at those times, unscaled.  The bands,
// the bit allocation and the dense mantissa planes (stride fullLines) stay the full shape's; a band that straddles the
// cut is dequantised on its lines below it.
__global__ __launch_bounds__(kThreads) void decode_reduced_kernel(DevShape R, const unsigned char* __restrict__ bandOfLine,
                                                                  int nb, int fullLines, int nScaleBits, int nStreams,
                                                                  const int* __restrict__ oscale,
                                                                  const int* __restrict__ msSwitch,
                                                                  const int* __restrict__ scaleFactor,
                                                                  const int* __restrict__ bitAlloc,
                                                                  const int* __restrict__ mantissa,
                                                                  const int64_t* __restrict__ outOffset,
                                                                  double* __restrict__ outL, double* __restrict__ outR) {
    extern __shared__ double smem[];
    const BlockChannel bc = block_channel(nStreams);
    decode_block<false>(R, bandOfLine, nb, fullLines, nScaleBits, nStreams == 2, bc.f, bc.ch, oscale, msSwitch, scaleFactor, bitAlloc,
                 mantissa, (bc.ch == 0 ? outL : outR) + outOffset[bc.f], smem);
}

__global__ __launch_bounds__(kThreads) void decode_reduced_mix_kernel(DevShape R, const unsigned char* __restrict__ bandOfLine,
                                                                      int nb, int fullLines, int nScaleBits, int joint,
                                                                      int mixSel, int64_t nPairs,
                                                                      const int* __restrict__ oscale,
                                                                      const int* __restrict__ msSwitch,
                                                                      const int* __restrict__ scaleFactor,
                                                                      const int* __restrict__ bitAlloc,
                                                                      const int* __restrict__ mantissa,
                                                                      const int64_t* __restrict__ outOffset,
                                                                      double* __restrict__ out) {
    extern __shared__ double smem[];
    int64_t f;
    int sel;
    mix_slot(joint != 0, mixSel, nPairs, &f, &sel);
    decode_block<true>(R, bandOfLine, nb, fullLines, nScaleBits, joint != 0, f, sel, oscale, msSwitch, scaleFactor, bitAlloc, mantissa,
                 out + outOffset[blockIdx.x], smem);
}

// The four store launches with band gains (mrc_pac_store_decode_window_shaped).  Sh: lineBand, the band of every line of the
// block's full shape; gain [units][nBands]; unit, the row of gains per slot (two-plane launches) or per workgroup (one-plane
// launches) -- indexed exactly as outOffset is.
struct ShapeDev {
    const unsigned short* lineBand;
    const double* gain;
    const int* unit;
    int nBands;
};
__device__ __forceinline__ const double* gain_row(const ShapeDev& Sh, int64_t at) { return Sh.gain + (int64_t)Sh.unit[at] * Sh.nBands; }

__global__ __launch_bounds__(kThreads) void decode_shaped_kernel(DevShape S, ShapeDev Sh, int nStreams,
                                                                 const int* __restrict__ oscale,
                                                                 const int* __restrict__ msSwitch,
                                                                 const int* __restrict__ scaleFactor,
                                                                 const int* __restrict__ bitAlloc,
                                                                 const int* __restrict__ mantissa,
                                                                 const int64_t* __restrict__ outOffset,
                                                                 double* __restrict__ outL, double* __restrict__ outR) {
    extern __shared__ double smem[];
    const BlockChannel bc = block_channel(nStreams);
    decode_block<false, true>(S, S.bandOfLine, S.nBands, S.halfN, S.nScaleBits, nStreams == 2, bc.f, bc.ch, oscale, msSwitch,
                              scaleFactor, bitAlloc, mantissa, (bc.ch == 0 ? outL : outR) + outOffset[bc.f], smem, Sh.lineBand,
                              gain_row(Sh, bc.f));
}

__global__ __launch_bounds__(kThreads) void decode_shaped_mix_kernel(DevShape S, ShapeDev Sh, int joint, int mixSel, int64_t nPairs,
                                                                     const int* __restrict__ oscale,
                                                                     const int* __restrict__ msSwitch,
                                                                     const int* __restrict__ scaleFactor,
                                                                     const int* __restrict__ bitAlloc,
                                                                     const int* __restrict__ mantissa,
                                                                     const int64_t* __restrict__ outOffset,
                                                                     double* __restrict__ out) {
    extern __shared__ double smem[];
    int64_t f;
    int sel;
    mix_slot(joint != 0, mixSel, nPairs, &f, &sel);
    decode_block<true, true>(S, S.bandOfLine, S.nBands, S.halfN, S.nScaleBits, joint != 0, f, sel, oscale, msSwitch, scaleFactor,
                             bitAlloc, mantissa, out + outOffset[blockIdx.x], smem, Sh.lineBand, gain_row(Sh, blockIdx.x));
}

__global__ __launch_bounds__(kThreads) void decode_reduced_shaped_kernel(DevShape R, ShapeDev Sh,
                                                                         const unsigned char* __restrict__ bandOfLine, int nb,
                                                                         int fullLines, int nScaleBits, int nStreams,
                                                                         const int* __restrict__ oscale,
                                                                         const int* __restrict__ msSwitch,
                                                                         const int* __restrict__ scaleFactor,
                                                                         const int* __restrict__ bitAlloc,
                                                                         const int* __restrict__ mantissa,
                                                                         const int64_t* __restrict__ outOffset,
                                                                         double* __restrict__ outL, double* __restrict__ outR) {
    extern __shared__ double smem[];
    const BlockChannel bc = block_channel(nStreams);
    decode_block<false, true>(R, bandOfLine, nb, fullLines, nScaleBits, nStreams == 2, bc.f, bc.ch, oscale, msSwitch, scaleFactor,
                              bitAlloc, mantissa, (bc.ch == 0 ? outL : outR) + outOffset[bc.f], smem, Sh.lineBand, gain_row(Sh, bc.f));
}

__global__ __launch_bounds__(kThreads) void decode_reduced_shaped_mix_kernel(DevShape R, ShapeDev Sh,
                                                                             const unsigned char* __restrict__ bandOfLine, int nb,
                                                                             int fullLines, int nScaleBits, int joint, int mixSel,
                                                                             int64_t nPairs, const int* __restrict__ oscale,
                                                                             const int* __restrict__ msSwitch,
                                                                             const int* __restrict__ scaleFactor,
                                                                             const int* __restrict__ bitAlloc,
                                                                             const int* __restrict__ mantissa,
                                                                             const int64_t* __restrict__ outOffset,
                                                                             double* __restrict__ out) {
    extern __shared__ double smem[];
    int64_t f;
    int sel;
    mix_slot(joint != 0, mixSel, nPairs, &f, &sel);
    decode_block<true, true>(R, bandOfLine, nb, fullLines, nScaleBits, joint != 0, f, sel, oscale, msSwitch, scaleFactor, bitAlloc,
                             mantissa, out + outOffset[blockIdx.x], smem, Sh.lineBand, gain_row(Sh, blockIdx.x));
}

// pcmfile.py:163-172
__global__ void pcm16_kernel(int64_t n, const double* __restrict__ x, short* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    const double mag = fabs(v);
    const int code = mag == 0.0 ? 0 : (int)mag_code(mag, 16);
    out[i] = (short)(signbit(v) ? -code : code);
}

}  // namespace

hipError_t launch_decode(const DevShape& S, int64_t nBlocks, int nStreams, const int* oscale, const int* msSwitch,
                         const int* scaleFactor, const int* bitAlloc, const int* mantissa, const int64_t* outOffset,
                         double* outL, double* outR, hipStream_t st) {
    if (nBlocks <= 0) return hipSuccess;
    const size_t lds = mdct_generic_lds_bytes(S);          // (the same [2N] doubles as mdct_kernel)
    hipLaunchKernelGGL(decode_kernel, dim3((unsigned)(nBlocks * nStreams)), dim3(kThreads), lds, st, S, nStreams, oscale,
                       msSwitch, scaleFactor, bitAlloc, mantissa, outOffset, outL, outR);
    return hipGetLastError();
}

hipError_t launch_decode_reduced(const DevShape& F, const DevShape& R, int64_t nBlocks, int nStreams, const int* oscale,
                                 const int* msSwitch, const int* scaleFactor, const int* bitAlloc, const int* mantissa,
                                 const int64_t* outOffset, double* outL, double* outR, hipStream_t st) {
    if (nBlocks <= 0) return hipSuccess;
    if (R.halfN <= 0 || R.halfN > F.halfN) return hipErrorInvalidValue;
    const size_t lds = mdct_generic_lds_bytes(R);
    hipLaunchKernelGGL(decode_reduced_kernel, dim3((unsigned)(nBlocks * nStreams)), dim3(kThreads), lds, st, R, F.bandOfLine,
                       F.nBands, F.halfN, F.nScaleBits, nStreams, oscale, msSwitch, scaleFactor, bitAlloc, mantissa, outOffset,
                       outL, outR);
    return hipGetLastError();
}

// One plane: F the block's full shape, R its reduced one (null: full rate, decode_mix_kernel).  nWorkgroups: the joint
// group's slots, or the non-joint group's nPairs pairs + single slots (2 nPairs + singles slots in all); mixSel: 0 / 1 / 2 =
// L / R / mid of a joint slot.  outOffset [nWorkgroups].
hipError_t launch_decode_mix(const DevShape& F, const DevShape* R, int64_t nWorkgroups, int joint, int mixSel, int64_t nPairs,
                             const int* oscale, const int* msSwitch, const int* scaleFactor, const int* bitAlloc,
                             const int* mantissa, const int64_t* outOffset, double* out, hipStream_t st) {
    if (nWorkgroups <= 0) return hipSuccess;
    if (mixSel < 0 || mixSel > kSelMid || nPairs < 0 || nPairs > nWorkgroups || (joint && nPairs) || nWorkgroups > 0x7fffffffLL)
        return hipErrorInvalidValue;
    if (!R) {
        hipLaunchKernelGGL(decode_mix_kernel, dim3((unsigned)nWorkgroups), dim3(kThreads), mdct_generic_lds_bytes(F), st, F, joint,
                           mixSel, nPairs, oscale, msSwitch, scaleFactor, bitAlloc, mantissa, outOffset, out);
        return hipGetLastError();
    }
    if (R->halfN <= 0 || R->halfN > F.halfN) return hipErrorInvalidValue;
    hipLaunchKernelGGL(decode_reduced_mix_kernel, dim3((unsigned)nWorkgroups), dim3(kThreads), mdct_generic_lds_bytes(*R), st, *R,
                       F.bandOfLine, F.nBands, F.halfN, F.nScaleBits, joint, mixSel, nPairs, oscale, msSwitch, scaleFactor,
                       bitAlloc, mantissa, outOffset, out);
    return hipGetLastError();
}

// launch_decode / launch_decode_reduced (R null: full rate) with band gains: one gain per line of the block's full shape F
// before the inverse transform.  lineBand [F.halfN] (kNoLineBand: the line is left alone), gain [units][nBands],
// unit [nBlocks] (a slot's row of gain, indexed as outOffset), all DEVICE.
hipError_t launch_decode_shaped(const DevShape& F, const DevShape* R, const unsigned short* lineBand, const double* gain,
                                const int* unit, int nBands, int64_t nBlocks, int nStreams, const int* oscale, const int* msSwitch,
                                const int* scaleFactor, const int* bitAlloc, const int* mantissa, const int64_t* outOffset,
                                double* outL, double* outR, hipStream_t st) {
    if (nBlocks <= 0) return hipSuccess;
    if (!lineBand || !gain || !unit || nBands < 1) return hipErrorInvalidValue;
    const ShapeDev Sh{lineBand, gain, unit, nBands};
    if (!R) {
        hipLaunchKernelGGL(decode_shaped_kernel, dim3((unsigned)(nBlocks * nStreams)), dim3(kThreads), mdct_generic_lds_bytes(F), st,
                           F, Sh, nStreams, oscale, msSwitch, scaleFactor, bitAlloc, mantissa, outOffset, outL, outR);
        return hipGetLastError();
    }
    if (R->halfN <= 0 || R->halfN > F.halfN) return hipErrorInvalidValue;
    hipLaunchKernelGGL(decode_reduced_shaped_kernel, dim3((unsigned)(nBlocks * nStreams)), dim3(kThreads), mdct_generic_lds_bytes(*R),
                       st, *R, Sh, F.bandOfLine, F.nBands, F.halfN, F.nScaleBits, nStreams, oscale, msSwitch, scaleFactor, bitAlloc,
                       mantissa, outOffset, outL, outR);
    return hipGetLastError();
}

// launch_decode_mix with band gains; unit [nWorkgroups], per workgroup as outOffset is.
hipError_t launch_decode_shaped_mix(const DevShape& F, const DevShape* R, const unsigned short* lineBand, const double* gain,
                                    const int* unit, int nBands, int64_t nWorkgroups, int joint, int mixSel, int64_t nPairs,
                                    const int* oscale, const int* msSwitch, const int* scaleFactor, const int* bitAlloc,
                                    const int* mantissa, const int64_t* outOffset, double* out, hipStream_t st) {
    if (nWorkgroups <= 0) return hipSuccess;
    if (mixSel < 0 || mixSel > kSelMid || nPairs < 0 || nPairs > nWorkgroups || (joint && nPairs) || nWorkgroups > 0x7fffffffLL)
        return hipErrorInvalidValue;
    if (!lineBand || !gain || !unit || nBands < 1) return hipErrorInvalidValue;
    const ShapeDev Sh{lineBand, gain, unit, nBands};
    if (!R) {
        hipLaunchKernelGGL(decode_shaped_mix_kernel, dim3((unsigned)nWorkgroups), dim3(kThreads), mdct_generic_lds_bytes(F), st, F, Sh,
                           joint, mixSel, nPairs, oscale, msSwitch, scaleFactor, bitAlloc, mantissa, outOffset, out);
        return hipGetLastError();
    }
    if (R->halfN <= 0 || R->halfN > F.halfN) return hipErrorInvalidValue;
    hipLaunchKernelGGL(decode_reduced_shaped_mix_kernel, dim3((unsigned)nWorkgroups), dim3(kThreads), mdct_generic_lds_bytes(*R), st,
                       *R, Sh, F.bandOfLine, F.nBands, F.halfN, F.nScaleBits, joint, mixSel, nPairs, oscale, msSwitch, scaleFactor,
                       bitAlloc, mantissa, outOffset, out);
    return hipGetLastError();
}

hipError_t launch_pcm16(int64_t n, const double* x, short* out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(pcm16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, x, out);
    return hipGetLastError();
}

}  // namespace mrc
