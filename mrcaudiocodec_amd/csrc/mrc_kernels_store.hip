// Windows of resident `.pac` files on gfx950 (mrc_pac_store_decode_window, mrc_api_store.cpp).
//
//   window_out_kernel   the margin planes decode_kernel added the windows' blocks to -> out [item][channel][t] in the
//     caller's format.  A row is one (item, output channel); a workgroup takes 256 consecutive t of one row, so a wave
//     reads 64 consecutive doubles of one plane and stores 64 consecutive values: both sides coalesced.  Row and tile come
//     from the workgroup's index (two divisions per workgroup, none per element, no search).  Sample t of the window is
//     plane[2 L + t]; where start + t lies outside the file the value is +0.0 and the plane is not read.  A one-channel
//     item fills every output channel from its one plane.
//       MRC_WINDOW_F64    the plane's value as it is: the same at most two contributions added to zero that the whole-file
//                         decode adds, so the same bits;
//       MRC_WINDOW_F32    (float) of it, one conversion, round to nearest even;
//       MRC_WINDOW_PCM16  pcmfile.py:163-172 exactly as pcm16_kernel (mrc_kernels_decode.hip) has it.
//
//   block_energy_kernel   the energy a block adds to the decoded signal, from its MDCT lines alone
//     (mrc_pac_store_block_energy).  The windowed MDCT with the codec's transition windows is an orthogonal lapped
//     transform; with the reference's scaling (mdct.py: forward 2 / N, inverse 2) a block of shape (a, b) holds
//     (a + b) sum_k x^[k]^2 of the signal's sum of squares, and at 1 / D of the rate its first n = (a + b) / (2 D) lines hold
//       e = ((a + b) / D) * sum_{k < n} x^[k]^2
//     of the reduced signal's.  x^[k] is decode_line's value for a channel and decode_line_mid's for the mid -- the lines
//     decode_kernel and decode_reduced_kernel transform, bands and line stride the full shape's, a band that straddles
//     the cut counted on its lines below it; the mid of a stereo file's last block, two non-joint slots side by side, is
//     0.5 * (x0 + x1) as in decode_block.  No inverse transform, no plane, no LDS.
//     One wave of 64 lanes per entry (a block's channel, or its mid), four entries per workgroup; the entry names its
//     slot, so nothing depends on how the slots are laid out.  A wave reads 64 consecutive mantissa codes per step.
//     Determinism: every sum has one fixed order.  Lane l adds the squares x^[k]^2 of lines k = l, l + 64, l + 128, ...
//     one after the other in ascending k, starting from +0.0 (a square is rounded once, then added: no fused
//     multiply-add).  The 64 lane sums then go through one fixed balanced tree over the lanes in their natural order
//     (wave_sum: lanes 2 i and 2 i + 1, then neighbouring pairs, quads, groups of 8, rows of 16, halves of 32 -- every
//     step adds two values that hold the same kind of partial sum, and a + b == b + a, so every lane ends with the same
//     bits), and lane 0 multiplies once by (a + b) / D, an integer.  Lanes past n contribute +0.0.  Nothing depends on
//     the grid, on which entries share the launch, on their order or on the slab.  No floating-point atomics.
#include "mrc_decode_lines.hpp"

namespace mrc {
using namespace dev;
namespace {

constexpr int kWindowThreads = 256;

__global__ __launch_bounds__(kWindowThreads) void window_out_kernel(const WindowItem* __restrict__ items, int64_t window,
                                                                    int64_t tiles, int nchOut, int format, int L,
                                                                    const double* __restrict__ planes,
                                                                    void* __restrict__ out) {
    const int64_t row = (int64_t)blockIdx.x / tiles;                 // item * nchOut + channel
    const int64_t t = ((int64_t)blockIdx.x - row * tiles) * kWindowThreads + threadIdx.x;
    if (t >= window) return;
    const int64_t k = row / nchOut;
    const int c = (int)(row - k * nchOut);
    const WindowItem it = items[k];
    const int64_t pos = it.start + t;
    double v = 0.0;
    if (pos >= 0 && pos < it.nSamples)
        v = planes[it.plane + (int64_t)(it.nch == 2 ? c : 0) * (window + 4 * (int64_t)L) + 2 * (int64_t)L + t];
    const int64_t o = row * window + t;
    if (format == MRC_WINDOW_F64) {
        ((double*)out)[o] = v;
    } else if (format == MRC_WINDOW_F32) {
        ((float*)out)[o] = (float)v;
    } else {
        const double mag = fabs(v);
        const int code = mag == 0.0 ? 0 : (int)mag_code(mag, 16);
        ((short*)out)[o] = (short)(signbit(v) ? -code : code);
    }
}

constexpr int kEnergyThreads = 256, kEnergyWave = 64;

__global__ __launch_bounds__(kEnergyThreads) void block_energy_kernel(const unsigned char* __restrict__ bandOfLine, int nb,
                                                                     int fullLines, int nScaleBits, int joint, int nLines,
                                                                     double factor, int64_t nEntries,
                                                                     const EnergyEntry* __restrict__ entries,
                                                                     const int* __restrict__ oscale,
                                                                     const int* __restrict__ msSwitch,
                                                                     const int* __restrict__ scaleFactor,
                                                                     const int* __restrict__ bitAlloc,
                                                                     const int* __restrict__ mantissa,
                                                                     double* __restrict__ energy) {
    const int lane = threadIdx.x % kEnergyWave;
    const int64_t w = (int64_t)blockIdx.x * (kEnergyThreads / kEnergyWave) + threadIdx.x / kEnergyWave;
    if (w >= nEntries) return;                                       // (the whole wave)
    const EnergyEntry e = entries[w];
    const int64_t f = e.slot;
    const int nStreams = joint ? 2 : 1;
    const int* sf = scaleFactor + f * nStreams * nb;
    const int* ba = bitAlloc + f * nStreams * nb;
    const int* mant = mantissa + f * nStreams * (int64_t)fullLines;
    const int* os = oscale + f * (joint ? 4 : 1);
    const int* ms = joint ? msSwitch + f * nb : nullptr;
    double acc = 0.0;
    if (e.sel != kEnergyMid) {
        for (int k = lane; k < nLines; k += kEnergyWave) {
            const double x = decode_line(k, bandOfLine[k], e.sel, joint != 0, nb, fullLines, nScaleBits, os, ms, sf, ba, mant);
            acc += x * x;
        }
    } else if (joint) {
        for (int k = lane; k < nLines; k += kEnergyWave) {
            const double x = decode_line_mid(k, bandOfLine[k], nb, fullLines, nScaleBits, os, ms, sf, ba, mant);
            acc += x * x;
        }
    } else {                                                         // slots f, f + 1: the two channels of a stereo file's last block
        for (int k = lane; k < nLines; k += kEnergyWave) {
            const int band = bandOfLine[k];
            const double x0 = decode_line(k, band, 0, false, nb, fullLines, nScaleBits, os, nullptr, sf, ba, mant);
            const double x1 = decode_line(k, band, 0, false, nb, fullLines, nScaleBits, os + 1, nullptr, sf + nb, ba + nb,
                                          mant + fullLines);
            const double x = 0.5 * (x0 + x1);
            acc += x * x;
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) energy[e.out] = factor * acc;
}

}  // namespace

hipError_t launch_window_out(int64_t nItems, const WindowItem* items, int64_t window, int nchOut, int format, int L,
                             const double* planes, void* out, hipStream_t st) {
    if (nItems <= 0 || window <= 0) return hipSuccess;
    const int64_t tiles = (window + kWindowThreads - 1) / kWindowThreads;
    const int64_t blocks = tiles * nItems * nchOut;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;          // (the caller cuts such a call into slabs)
    hipLaunchKernelGGL(window_out_kernel, dim3((unsigned)blocks), dim3(kWindowThreads), 0, st, items, window, tiles, nchOut,
                       format, L, planes, out);
    return hipGetLastError();
}

// F: the blocks' full shape; D: the rate divisor (1, 2 or 4, dividing F.halfN); the group's parsed arrays; entries (device)
// [nEntries], each writing energy[entry.out]
hipError_t launch_block_energy(const DevShape& F, int D, int joint, int64_t nEntries, const EnergyEntry* entries,
                               const int* oscale, const int* msSwitch, const int* scaleFactor, const int* bitAlloc,
                               const int* mantissa, double* energy, hipStream_t st) {
    if (nEntries <= 0) return hipSuccess;
    const int perGroup = kEnergyThreads / kEnergyWave;
    const int64_t blocks = (nEntries + perGroup - 1) / perGroup;
    if (D <= 0 || F.halfN % D || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(block_energy_kernel, dim3((unsigned)blocks), dim3(kEnergyThreads), 0, st, F.bandOfLine, F.nBands, F.halfN,
                       F.nScaleBits, joint, F.halfN / D, (double)(F.N / D), nEntries, entries, oscale, msSwitch, scaleFactor,
                       bitAlloc, mantissa, energy);
    return hipGetLastError();
}

}  // namespace mrc
