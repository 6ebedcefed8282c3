// The decoded MDCT lines of one channel of one block, before the IMDCT: shared by decode_kernel (mrc_kernels_decode.hip),
// nmr_band_kernel (mrc_kernels_nmr.hip) and nmr_rungs_kernel (mrc_kernels_target.hip), so that the noise the NMR measures is that of the samples the decoder writes.
//   vDequantize (quantize.py:325-357, operation order kept: ((sign*mag)*2) / (2^R - 1), one correctly rounded division)
//   -> divide by the overall scale level (a power of two: exact, codecThem.py:47-51, 92-109) -> ReconstructLR
//   (ms_stereo.py:33-49; a joint block's output channel dequantises BOTH streams of the bands whose M/S switch is set).
#pragma once
#include "mrc_device.hpp"

namespace mrc {
namespace dev {

// quantize.py:325-357 + 90-111 for one mantissa code
__device__ __forceinline__ double dequantize_dev(int scale, int mant, int nScaleBits, int nMantBits) {
    const int cap = (1 << nScaleBits) - 1;
    const int nBits = cap + nMantBits;
    const int signBit = 1 << (nMantBits - 1);
    const bool neg = mant >= signBit;
    const long long mag = neg ? mant - signBit : mant;
    long long code = mag;
    if (scale != cap) {
        const int shift = cap - scale;
        code = mag << shift;
        if (shift > 0 && mag > 0) code += 1LL << (shift - 1);
    }
    const double sgn = neg ? -1.0 : 1.0;
    return ((sgn * (double)code) * 2.0) / ((double)(1LL << nBits) - 1.0);
}

// Line k (band `band`) of output channel ch.  Non-joint: os[0], sf / ba [nb], mant [M] of the channel's own chunk.
// Joint: os [4] = L, R, M, S; ms [nb]; sf / ba [2][nb], mant [2][M] of the block's two streams.
// MantT: int (the parsed chunks of decode_kernel and nmr_band_kernel) or unsigned short (the chained scan's plane,
// nmr_rungs_kernel): the same codes.
template <class MantT>
__device__ __forceinline__ double decode_line(int k, int band, int ch, bool joint, int nb, int M, int nScaleBits,
                                              const int* __restrict__ os, const int* __restrict__ ms,
                                              const int* __restrict__ sf, const int* __restrict__ ba,
                                              const MantT* __restrict__ mant) {
    double x;
    if (!joint) {
        const int bits = ba[band];
        x = bits ? dequantize_dev(sf[band], mant[k], nScaleBits, bits) : 0.0;
        x = ldexp(x, -os[0]);
    } else {
        const bool isMs = ms[band] == 1;
        const int b0 = ba[band], b1 = ba[nb + band];
        double l1 = b0 ? ldexp(dequantize_dev(sf[band], mant[k], nScaleBits, b0), -(isMs ? os[2] : os[0])) : 0.0;
        double l2 = b1 ? ldexp(dequantize_dev(sf[nb + band], mant[M + k], nScaleBits, b1), -(isMs ? os[3] : os[1])) : 0.0;
        x = isMs ? (ch == 0 ? l1 + l2 : l1 - l2) : (ch == 0 ? l1 : l2);
    }
    return x;
}

// Line k of the MID (L + R) / 2 of a joint block (the store's mix windows, decode_mix_kernel): where the band's M/S switch
// is set the first stream IS the mid and the side stream is not dequantised at all; elsewhere 0.5 * (l1 + l2), l1 and l2
// as above.  (By linearity the inverse transform of these lines is the mean of the two channels' signals.)
__device__ __forceinline__ double decode_line_mid(int k, int band, int nb, int M, int nScaleBits, const int* __restrict__ os,
                                                  const int* __restrict__ ms, const int* __restrict__ sf,
                                                  const int* __restrict__ ba, const int* __restrict__ mant) {
    const bool isMs = ms[band] == 1;
    const int b0 = ba[band];
    const double l1 = b0 ? ldexp(dequantize_dev(sf[band], mant[k], nScaleBits, b0), -(isMs ? os[2] : os[0])) : 0.0;
    if (isMs) return l1;
    const int b1 = ba[nb + band];
    const double l2 = b1 ? ldexp(dequantize_dev(sf[nb + band], mant[M + k], nScaleBits, b1), -os[1]) : 0.0;
    return 0.5 * (l1 + l2);
}

}  // namespace dev
}  // namespace mrc
