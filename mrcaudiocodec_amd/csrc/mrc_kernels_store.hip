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
#include "mrc_device.hpp"

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

}  // namespace mrc
