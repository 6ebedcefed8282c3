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
//   resample_out_kernel   window_out_kernel's place in mrc_pac_store_decode_window_resampled: the planes hold the items'
//     INTERMEDIATE samples y (the signal at 1 / D of the file's rate), out the signal at up / down of that rate.  Output n of a
//     row sits at intermediate time n down / up; with q = floor(n down / up), p = n down mod up
//       v[n] = the left fold from +0.0 over j = 0 .. 2 W - 1 ascending of taps[p][j] * y[q - W + 1 + j],
//     every product rounded once, then added (__dmul_rn, __dadd_rn: no fused multiply-add), y +0.0 outside [0, nSamples).
//     A row is one (item, output channel); a workgroup of 256 threads takes 256 consecutive n of it.  What they read is one
//     run of at most 255 down / up + 2 W + 1 <= 4089 intermediate samples: all threads stage it into LDS with consecutive
//     loads of the plane (the file mask applied there, so the plane is not read outside the file), then each thread folds
//     from LDS, eight taps and samples read ahead of their additions.  The taps lie [tap][phase] in device memory, so that at
//     tap j a wave's 64 reads fall into one row of `up` doubles; for up == 1 and up == 2 the row is read at addresses the
//     whole wave shares (scalar loads) and each lane picks its phase's tap, in instantiations of their own.
//     LDS layout: at tap j lane k of a half wave reads run[o + floor((p0 + k down) / up)] with a 64-bit read, 32 lanes over
//     32 banks of a double.  down <= up, or down / up an odd whole number: 32 different banks, nothing to do.  Otherwise two
//     remedies, chosen per ratio on the host by counting (resample_lds_layout, mrc_resample_taps.hpp): skew -- double i
//     kept at i + (i >> 5), one double of padding per bank row, which takes the 2-, 4- and 8-way conflicts of the strides 2,
//     4 and 8 to under two cycles a read -- and evenOdd -- a wave's first half takes the even, its second half the odd of
//     its 64 outputs, so that a half's stride is 2 down / up: 3 / 2 becomes the odd stride 3, conflict-free.  Ratios like
//     441 / 160 keep their two cycles a read under all four layouts (DESIGN.md has the table).  A wave's stores are the
//     same 64 consecutive values either way.
//     Nothing depends on the grid, on the order of the items, on which items share the launch or on the slab.
//
//   sum_out_kernel, resample_sum_out_kernel   the two kernels above where a row is a weighted sum of windows
//     (mrc_pac_store_decode_window_sum).  Item i owns the term records [termOffset[i], termOffset[i + 1]): a WindowItem (the
//     term's plane, start and file length), its gain and, when resampling, its first output sample.  With v_k[t] what
//     window_out_kernel / resample_out_kernel would write as float64 for term k alone,
//       out[t] = the left fold from +0.0 over the item's terms IN THEIR ORDER of gain_k * v_k[t],
//     every product rounded once, then added (__dmul_rn, __dadd_rn); the caller's format is taken from the sum.  Rows, tiles
//     and the lane-to-output map are those of the kernel each stands for.  The term records are read at addresses made of
//     the workgroup's index and the loop counter alone: the same for every lane, so they stay in scalar registers.
//     sum_out_kernel loads four terms' samples ahead of their four additions (the additions keep their order; otherwise a
//     row of K terms is K HBM round trips one after the other), a wave reading 64 consecutive doubles of each plane; no LDS.
//     resample_sum_out_kernel stages one term's run of intermediate samples at a time (the file mask applied there), folds it
//     with resample_fold_up -- phase and first tap differ per term -- and adds gain * v between two barriers, the second
//     because the next term's run overwrites this one's; a term without a plane skips both, the whole workgroup together.
//     No atomics; nothing depends on the grid, on the order of the items, on what shares the launch or on the slab.
//
//   resample_multi_sum_out_kernel   resample_sum_out_kernel with the ratio read per term (mrc_pac_store_decode_window_speeds):
//     term j is read at ratios[ratioOf[j]], a SpeedRatio (up, down, W, skew, taps) at an address made of the workgroup's index
//     and the loop counter alone, so the record stays in scalar registers like the term's and every branch on it is taken by
//     the whole workgroup.  A non-unit ratio stages its run with that ratio's skew and folds it with resample_fold_up between
//     the two barriers, exactly as above; the unit ratio (W == 0) has no run: its value is sum_term_sample's, the plane at
//     2 L + t, and the workgroup skips both barriers together.  A thread's accumulator belongs to ONE output over all terms
//     of its row, so the lane-to-output map is the launch's, not the ratio's: the natural one (lane l takes output l), and each
//     ratio's skew is chosen for that map on the host.  A fold's order is per output, so the bits are those of the
//     single-ratio kernels whatever the map; only the LDS cycles of ratios that would take evenOdd (3 / 2) differ.
//     The taps pointer is read out of the record, where the single-ratio kernels have it as a kernel argument: a pointer out
//     of memory is a generic one to the compiler, and the fold's tap loads would become flat vector loads, one per lane, also
//     for up == 1 and up == 2.  So the fold takes its pointer type as a template argument and this kernel hands it a pointer
//     to the global address space (GlobalTaps): tap rows of up == 1 and up == 2 are scalar loads again, the general case
//     global loads -- the same mix of loads as resample_sum_out_kernel has.
//
//   The tile sizes, floor_div, the polyphase fold (resample_fold, resample_fold_up) and the sums' read-ahead live in
//   mrc_store_fold.hpp, which the span forms of the three folding kernels (mrc_kernels_store_span.hip) include as well.
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
//
//   band_energy_kernel   block_energy_kernel's sum split by frequency band (mrc_pac_store_band_energy_window):
//       B[entry][q] = sum of x^[k]^2 over lineLo[q] <= k < lineLo[q + 1],
//     x^ the same lines, lineLo the shape's table of mrc_band_line_ranges.  The CONTRACT is the order: each band is a left
//     fold from +0.0 over k ascending, every square rounded once, then added (no fused multiply-add) -- so a band cannot be
//     spread over lanes, and the parallelism lies across bands and entries.  One workgroup of 256 threads per entry, in two
//     phases per chunk of kBandChunk = 512 lines: all threads dequantise and square lines k = t, t + 256, ... into LDS (a
//     wave reads 64 consecutive mantissa codes per step, as block_energy_kernel does; a line is decoded once, whatever
//     the bands), then thread q continues band q's fold over the part of [lineLo[q], lineLo[q + 1]) inside the chunk,
//     its sum in a register from chunk to chunk, reading eight squares ahead of their additions (the additions keep their
//     order; without that every line costs an LDS round trip in the longest band's chain, 363 lines of a long block's
//     last critical band, which every other thread of the workgroup waits for).  A long block of 1024 lines is two
//     chunks, one of 8192 lines sixteen, in 4 KiB of LDS whatever the shape.  An empty band is +0.0; lines outside
//     every band are decoded and not read.  Nothing depends on the grid, on which entries share the launch or on their
//     order.
//
//   filterbank_energy_kernel   band_energy_kernel with a weight per line and filter (mrc_pac_store_filterbank_window):
//       F[entry][q] = sum of w_q[k] * x^[k]^2 over lo[q] <= k < hi[q],
//     the filters triangles that overlap, w_q, lo and hi the shape's table of mrc_filterbank_line_weights (host float64).
//     The CONTRACT is again the order: a left fold from +0.0 over k ascending, the square rounded once, the product rounded
//     once, then added (__dmul_rn, __dadd_rn: no fused multiply-add) -- a filter cannot be spread over lanes.  The band
//     kernel's shape: one workgroup of 256 threads per entry, the chunk's squares staged in LDS (a line is decoded once
//     however many filters it feeds: two inside a bank, more where filters are narrower than a line), thread q continuing
//     filter q's fold through the chunk with its sum in a register, eight squares AND eight weights read ahead of their
//     additions.  The weights are not staged: thread q walks its own row in global memory, weight[off[q] + (k - lo[q])], eight
//     consecutive doubles per step.  A shape's rows are under 20 KiB (at most 2 halfN + 2 nFilters weights), the same for
//     every workgroup of the launch, so after the first they come from L2; neighbouring threads' addresses lie a row
//     apart, which costs a cache line per thread and step where LDS staging would cost a second barrier pair and, for
//     overlapping rows, an LDS layout per chunk.  Rows are short (89 lines at most for 80 mel filters on 1024 lines, the band
//     kernel's longest chain is 363), so the fold is shorter than the band kernel's however the weights arrive.  tab is
//     int32 [3][nFilters]: lo, hi, off.  An empty row (a filter wholly above the last line) is +0.0.  Nothing depends on
//     the grid, on which entries share the launch or on their order.
//
//   band_frames_kernel   B laid on the call's frame grid.  One thread per output value, frames fastest -- the flat index
//     is the output's own, so a wave stores 64 consecutive values -- and a row is (item, output channel, band).  The
//     item's needed blocks are abutting tiles in DOUBLED output samples (a tile edge is a half sample); the thread finds
//     the first tile that ends behind its frame's start by bisection, then folds forward from +0.0 while tiles start
//     before the frame's end: acc += (double)ov2 * B, ov2 = 2 |tile and frame| > 0 an exact integer.  A frame that meets
//     no tile is +0.0.  MRC_WINDOW_F32 converts acc once.  No atomics; nothing depends on the grid or the slab.
#include "mrc_decode_lines.hpp"
#include "mrc_store_fold.hpp"

namespace mrc {
using namespace dev;
namespace {

// (store_window_value, out[o] = v in the caller's format: mrc_device.hpp, shared with mrc_kernels_reverb.hip)

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
    store_window_value(out, row * window + t, format, v);
}

__global__ __launch_bounds__(kResampleThreads) void resample_out_kernel(const WindowItem* __restrict__ items,
                                                                        const long long* __restrict__ outStart, int64_t window,
                                                                        int64_t tiles, int nchOut, int format, int L,
                                                                        int64_t planeLen, int up, int down, int W, int evenOdd,
                                                                        int skew, const double* __restrict__ taps,
                                                                        const double* __restrict__ planes,
                                                                        void* __restrict__ out) {
    __shared__ double run[kResampleLds];
    const int64_t row = (int64_t)blockIdx.x / tiles;                 // item * nchOut + channel
    const int64_t t0 = ((int64_t)blockIdx.x - row * tiles) * kResampleThreads;
    const int64_t k = row / nchOut;
    const int c = (int)(row - k * nchOut);
    const WindowItem it = items[k];
    // the thread's output: lane l of a wave takes output l of the wave's 64, or (evenOdd) its first half the even and its
    // second half the odd ones -- a wave's stores cover the same 64 consecutive values either way
    const int lane = threadIdx.x % kResampleWave, wave = threadIdx.x / kResampleWave;
    const int64_t t = t0 + wave * kResampleWave + (evenOdd ? 2 * (lane & 31) + (lane >> 5) : lane);
    if (it.nSamples == 0) {                                          // (the whole workgroup) no plane: every y is +0.0
        if (t < window) store_window_value(out, row * window + t, format, 0.0);
        return;
    }
    // the run of intermediate samples the tile's outputs read: [qFirst, qFirst + len)
    const int64_t n0 = outStart[k] + t0, nLast = n0 + min((int64_t)kResampleThreads, window - t0) - 1;
    const int64_t qFirst = floor_div(n0 * down, up) - W + 1;
    const int len = (int)(floor_div(nLast * down, up) + W - qFirst + 1);       // <= kResampleRun (the launcher's check)
    const double* plane = planes + it.plane + (int64_t)(it.nch == 2 ? c : 0) * planeLen;
    for (int i = threadIdx.x; i < len; i += kResampleThreads) {
        const int64_t m = qFirst + i, at = 2 * (int64_t)L + (m - it.start);   // y[m] is plane[2 L + m - start] inside the file
        double v = 0.0;
        if (m >= 0 && m < it.nSamples && at >= 0 && at < planeLen) v = plane[at];
        run[i + skew * (i >> 5)] = v;
    }
    __syncthreads();
    if (t >= window) return;
    const int64_t nd = (outStart[k] + t) * down, q = floor_div(nd, up);
    const int p = (int)(nd - q * up), first = (int)(q - W + 1 - qFirst);
    const double v = skew ? resample_fold_up<true>(taps, up, p, run, first, 2 * W) : resample_fold_up<false>(taps, up, p, run, first, 2 * W);
    store_window_value(out, row * window + t, format, v);
}

// window_out_kernel's value of one term at sample t of channel c: the plane's, +0.0 outside the file or without a plane
__device__ inline double sum_term_sample(const SumTerm& tm, int c, int64_t t, int64_t planeLen, int L,
                                         const double* __restrict__ planes) {
    const int64_t pos = tm.w.start + t;
    double y = 0.0;
    if (pos >= 0 && pos < tm.w.nSamples) y = planes[tm.w.plane + (int64_t)(tm.w.nch == 2 ? c : 0) * planeLen + 2 * (int64_t)L + t];
    return y;
}

__global__ __launch_bounds__(kWindowThreads) void sum_out_kernel(const SumTerm* __restrict__ terms,
                                                                 const long long* __restrict__ termOffset, int64_t window,
                                                                 int64_t tiles, int nchOut, int format, int L,
                                                                 const double* __restrict__ planes, void* __restrict__ out) {
    const int64_t row = (int64_t)blockIdx.x / tiles;                 // item * nchOut + channel
    const int64_t t = ((int64_t)blockIdx.x - row * tiles) * kWindowThreads + threadIdx.x;
    const int64_t k = row / nchOut;
    const int c = (int)(row - k * nchOut);
    // the item's terms: the same for the whole workgroup (indexed from blockIdx and the loop counter alone)
    const int64_t jEnd = termOffset[k + 1], planeLen = window + 4 * (int64_t)L;
    int64_t j = termOffset[k];
    if (t >= window) return;
    double acc = 0.0;
    for (; j + kSumAhead <= jEnd; j += kSumAhead) {
        double g[kSumAhead], y[kSumAhead];
#pragma unroll
        for (int u = 0; u < kSumAhead; ++u) {
            g[u] = terms[j + u].gain;
            y[u] = sum_term_sample(terms[j + u], c, t, planeLen, L, planes);
        }
#pragma unroll
        for (int u = 0; u < kSumAhead; ++u) acc = __dadd_rn(acc, __dmul_rn(g[u], y[u]));
    }
    for (; j < jEnd; ++j) acc = __dadd_rn(acc, __dmul_rn(terms[j].gain, sum_term_sample(terms[j], c, t, planeLen, L, planes)));
    store_window_value(out, row * window + t, format, acc);
}

__global__ __launch_bounds__(kResampleThreads) void resample_sum_out_kernel(const SumTerm* __restrict__ terms,
                                                                            const long long* __restrict__ termOffset,
                                                                            int64_t window, int64_t tiles, int nchOut, int format,
                                                                            int L, int64_t planeLen, int up, int down, int W,
                                                                            int evenOdd, int skew, const double* __restrict__ taps,
                                                                            const double* __restrict__ planes,
                                                                            void* __restrict__ out) {
    __shared__ double run[kResampleLds];
    const int64_t row = (int64_t)blockIdx.x / tiles;                 // item * nchOut + channel
    const int64_t t0 = ((int64_t)blockIdx.x - row * tiles) * kResampleThreads;
    const int64_t k = row / nchOut;
    const int c = (int)(row - k * nchOut);
    const int lane = threadIdx.x % kResampleWave, wave = threadIdx.x / kResampleWave;      // (resample_out_kernel's map)
    const int64_t t = t0 + wave * kResampleWave + (evenOdd ? 2 * (lane & 31) + (lane >> 5) : lane);
    const int64_t jEnd = termOffset[k + 1];
    double acc = 0.0;
    for (int64_t j = termOffset[k]; j < jEnd; ++j) {                 // (every branch on the term: the whole workgroup)
        const SumTerm tm = terms[j];
        if (tm.w.nSamples == 0) continue;                            // no plane: every y is +0.0, the term adds nothing
        // the term's run of intermediate samples under the tile's outputs: [qFirst, qFirst + len)
        const int64_t n0 = tm.outStart + t0, nLast = n0 + min((int64_t)kResampleThreads, window - t0) - 1;
        const int64_t qFirst = floor_div(n0 * down, up) - W + 1;
        const int len = (int)(floor_div(nLast * down, up) + W - qFirst + 1);   // <= kResampleRun (the launcher's check)
        const double* plane = planes + tm.w.plane + (int64_t)(tm.w.nch == 2 ? c : 0) * planeLen;
        for (int i = threadIdx.x; i < len; i += kResampleThreads) {
            const int64_t m = qFirst + i, at = 2 * (int64_t)L + (m - tm.w.start);
            double v = 0.0;
            if (m >= 0 && m < tm.w.nSamples && at >= 0 && at < planeLen) v = plane[at];
            run[i + skew * (i >> 5)] = v;
        }
        __syncthreads();
        if (t < window) {
            const int64_t nd = (tm.outStart + t) * down, q = floor_div(nd, up);
            const int p = (int)(nd - q * up), first = (int)(q - W + 1 - qFirst);
            const double v = skew ? resample_fold_up<true>(taps, up, p, run, first, 2 * W) : resample_fold_up<false>(taps, up, p, run, first, 2 * W);
            acc = __dadd_rn(acc, __dmul_rn(tm.gain, v));
        }
        __syncthreads();                                             // (the next term's run goes over this one)
    }
    if (t < window) store_window_value(out, row * window + t, format, acc);
}

__global__ __launch_bounds__(kResampleThreads) void resample_multi_sum_out_kernel(const SumTerm* __restrict__ terms,
                                                                                  const int* __restrict__ ratioOf,
                                                                                  const SpeedRatio* __restrict__ ratios,
                                                                                  const long long* __restrict__ termOffset,
                                                                                  int64_t window, int64_t tiles, int nchOut,
                                                                                  int format, int L, int64_t planeLen,
                                                                                  const double* __restrict__ planes,
                                                                                  void* __restrict__ out) {
    __shared__ double run[kResampleLds];
    const int64_t row = (int64_t)blockIdx.x / tiles;                 // item * nchOut + channel
    const int64_t t0 = ((int64_t)blockIdx.x - row * tiles) * kResampleThreads;
    const int64_t k = row / nchOut;
    const int c = (int)(row - k * nchOut);
    const int64_t t = t0 + threadIdx.x;                              // the natural map: the accumulator's output, whatever the term
    const int64_t jEnd = termOffset[k + 1];
    double acc = 0.0;
    for (int64_t j = termOffset[k]; j < jEnd; ++j) {                 // (every branch on the term or its ratio: the whole workgroup)
        const SumTerm tm = terms[j];
        if (tm.w.nSamples == 0) continue;                            // no plane: every y is +0.0, the term adds nothing
        const SpeedRatio r = ratios[ratioOf[j]];                     // (blockIdx and the loop counter alone: scalar)
        if (r.W == 0) {                                              // the unit ratio: sum_out_kernel's term, no LDS, no barrier
            if (t < window) acc = __dadd_rn(acc, __dmul_rn(tm.gain, sum_term_sample(tm, c, t, planeLen, L, planes)));
            continue;
        }
        const int up = r.up, down = r.down, W = r.W, skew = r.skew;
        // the taps pointer comes out of memory: said to be a global one, as a kernel argument is known to be, so that the
        // up == 1 and up == 2 folds read their tap rows with scalar loads and the general one with global loads
        const GlobalTaps taps = (GlobalTaps)r.taps;
        // the term's run of intermediate samples under the tile's outputs: [qFirst, qFirst + len)
        const int64_t n0 = tm.outStart + t0, nLast = n0 + min((int64_t)kResampleThreads, window - t0) - 1;
        const int64_t qFirst = floor_div(n0 * down, up) - W + 1;
        const int len = (int)(floor_div(nLast * down, up) + W - qFirst + 1);   // <= kResampleRun (the launcher's check)
        const double* plane = planes + tm.w.plane + (int64_t)(tm.w.nch == 2 ? c : 0) * planeLen;
        for (int i = threadIdx.x; i < len; i += kResampleThreads) {
            const int64_t m = qFirst + i, at = 2 * (int64_t)L + (m - tm.w.start);
            double v = 0.0;
            if (m >= 0 && m < tm.w.nSamples && at >= 0 && at < planeLen) v = plane[at];
            run[i + skew * (i >> 5)] = v;
        }
        __syncthreads();
        if (t < window) {
            const int64_t nd = (tm.outStart + t) * down, q = floor_div(nd, up);
            const int p = (int)(nd - q * up), first = (int)(q - W + 1 - qFirst);
            const double v = skew ? resample_fold_up<true>(taps, up, p, run, first, 2 * W) : resample_fold_up<false>(taps, up, p, run, first, 2 * W);
            acc = __dadd_rn(acc, __dmul_rn(tm.gain, v));
        }
        __syncthreads();                                             // (the next term's run goes over this one)
    }
    if (t < window) store_window_value(out, row * window + t, format, acc);
}

constexpr int kEnergyThreads = 256, kEnergyWave = 64;

// The parsed arrays of one EnergyEntry and line k as the entry selects it: a channel's decode_line, the mid's
// decode_line_mid, or for the pair of non-joint slots of a stereo file's last block 0.5 * (x0 + x1) as in decode_block.
struct EntryLines {
    const unsigned char* bandOfLine;
    const int *os, *ms, *sf, *ba, *mant;
    int nb, fullLines, nScaleBits, sel;
    bool joint;
    __device__ EntryLines(const EnergyEntry& e, const unsigned char* bandOfLine_, int nb_, int fullLines_, int nScaleBits_, int joint_,
                          const int* oscale, const int* msSwitch, const int* scaleFactor, const int* bitAlloc, const int* mantissa)
        : bandOfLine(bandOfLine_), nb(nb_), fullLines(fullLines_), nScaleBits(nScaleBits_), sel(e.sel), joint(joint_ != 0) {
        const int64_t f = e.slot;
        const int nStreams = joint ? 2 : 1;
        sf = scaleFactor + f * nStreams * nb;
        ba = bitAlloc + f * nStreams * nb;
        mant = mantissa + f * nStreams * (int64_t)fullLines;
        os = oscale + f * (joint ? 4 : 1);
        ms = joint ? msSwitch + f * nb : nullptr;
    }
    __device__ double line(int k) const {
        const int band = bandOfLine[k];
        if (sel != kEnergyMid) return decode_line(k, band, sel, joint, nb, fullLines, nScaleBits, os, ms, sf, ba, mant);
        if (joint) return decode_line_mid(k, band, nb, fullLines, nScaleBits, os, ms, sf, ba, mant);
        const double x0 = decode_line(k, band, 0, false, nb, fullLines, nScaleBits, os, nullptr, sf, ba, mant);
        const double x1 = decode_line(k, band, 0, false, nb, fullLines, nScaleBits, os + 1, nullptr, sf + nb, ba + nb, mant + fullLines);
        return 0.5 * (x0 + x1);
    }
};

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
    const EntryLines L(e, bandOfLine, nb, fullLines, nScaleBits, joint, oscale, msSwitch, scaleFactor, bitAlloc, mantissa);
    double acc = 0.0;
    for (int k = lane; k < nLines; k += kEnergyWave) {
        const double x = L.line(k);
        acc += x * x;
    }
    acc = wave_sum(acc);
    if (lane == 0) energy[e.out] = factor * acc;
}

constexpr int kBandThreads = 256, kBandChunk = 512;

__global__ __launch_bounds__(kBandThreads) void band_energy_kernel(const unsigned char* __restrict__ bandOfLine, int nb,
                                                                  int fullLines, int nScaleBits, int joint, int nBands,
                                                                  const int* __restrict__ lineLo, int64_t nEntries,
                                                                  const EnergyEntry* __restrict__ entries,
                                                                  const int* __restrict__ oscale,
                                                                  const int* __restrict__ msSwitch,
                                                                  const int* __restrict__ scaleFactor,
                                                                  const int* __restrict__ bitAlloc,
                                                                  const int* __restrict__ mantissa,
                                                                  double* __restrict__ bandSums) {
    __shared__ double sq[kBandChunk];
    const int t = threadIdx.x;
    const EnergyEntry e = entries[blockIdx.x];
    const EntryLines L(e, bandOfLine, nb, fullLines, nScaleBits, joint, oscale, msSwitch, scaleFactor, bitAlloc, mantissa);
    // thread t folds band t (nBands <= MRC_MAX_STORE_BANDS = kBandThreads: the launcher refuses more)
    const int lo = t < nBands ? lineLo[t] : 0, hi = t < nBands ? lineLo[t + 1] : 0;
    double acc = 0.0;
    for (int c0 = 0; c0 < fullLines; c0 += kBandChunk) {
        const int c1 = min(c0 + kBandChunk, fullLines);
        if (c0) __syncthreads();                                     // (the folds of the chunk before are done with sq)
        for (int k = c0 + t; k < c1; k += kBandThreads) {
            const double x = L.line(k);
            sq[k - c0] = x * x;
        }
        __syncthreads();
        // the fold, in order; eight squares are read ahead of their additions (one LDS round trip per eight, not per line)
        int k = max(lo, c0);
        const int kEnd = min(hi, c1);
        for (; k + 8 <= kEnd; k += 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = sq[k - c0 + u];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += v[u];
        }
        for (; k < kEnd; ++k) acc += sq[k - c0];
    }
    if (t < nBands) bandSums[e.out * nBands + t] = acc;
}

// tab: the shape's int32 [3][nFilters] -- lo, hi and the offset of filter q's row in weight; weight[offset + (k - lo)] is
// line k's weight in filter q (mrc_filterbank_line_weights).  hi <= fullLines.
__global__ __launch_bounds__(kBandThreads) void filterbank_energy_kernel(const unsigned char* __restrict__ bandOfLine, int nb,
                                                                        int fullLines, int nScaleBits, int joint, int nFilters,
                                                                        const int* __restrict__ tab,
                                                                        const double* __restrict__ weight, int64_t nEntries,
                                                                        const EnergyEntry* __restrict__ entries,
                                                                        const int* __restrict__ oscale,
                                                                        const int* __restrict__ msSwitch,
                                                                        const int* __restrict__ scaleFactor,
                                                                        const int* __restrict__ bitAlloc,
                                                                        const int* __restrict__ mantissa,
                                                                        double* __restrict__ filterSums) {
    __shared__ double sq[kBandChunk];
    const int t = threadIdx.x;
    const EnergyEntry e = entries[blockIdx.x];
    const EntryLines L(e, bandOfLine, nb, fullLines, nScaleBits, joint, oscale, msSwitch, scaleFactor, bitAlloc, mantissa);
    // thread t folds filter t (nFilters <= MRC_MAX_STORE_BANDS = kBandThreads: the launcher refuses more)
    const bool mine = t < nFilters;
    const int lo = mine ? tab[t] : 0, hi = mine ? min(tab[nFilters + t], fullLines) : 0;
    const int rel = (mine ? tab[2 * nFilters + t] : 0) - lo;         // weight[rel + k]: line k's weight
    double acc = 0.0;
    for (int c0 = 0; c0 < fullLines; c0 += kBandChunk) {
        const int c1 = min(c0 + kBandChunk, fullLines);
        if (c0) __syncthreads();                                     // (the folds of the chunk before are done with sq)
        for (int k = c0 + t; k < c1; k += kBandThreads) {
            const double x = L.line(k);
            sq[k - c0] = x * x;
        }
        __syncthreads();
        // the fold, in order: the product rounded once, then added; eight squares and eight weights are read ahead of their
        // additions (one LDS and one memory round trip per eight lines, not per line)
        int k = max(lo, c0);
        const int kEnd = min(hi, c1);
        for (; k + 8 <= kEnd; k += 8) {
            double v[8], wt[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                v[u] = sq[k - c0 + u];
                wt[u] = weight[rel + k + u];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = __dadd_rn(acc, __dmul_rn(wt[u], v[u]));
        }
        for (; k < kEnd; ++k) acc = __dadd_rn(acc, __dmul_rn(weight[rel + k], sq[k - c0]));
    }
    if (mine) filterSums[e.out * nFilters + t] = acc;
}

constexpr int kFrameThreads = 256;

__global__ __launch_bounds__(kFrameThreads) void band_frames_kernel(const BandItem* __restrict__ items,
                                                                   const long long* __restrict__ edges, int64_t total,
                                                                   int64_t nFrames, int64_t hop, int nBands, int nchOut,
                                                                   int format, const double* __restrict__ bandSums,
                                                                   void* __restrict__ out) {
    const int64_t o = (int64_t)blockIdx.x * kFrameThreads + threadIdx.x;      // out's own index: [item][channel][band][frame]
    if (o >= total) return;
    const int64_t row = o / nFrames, j = o - row * nFrames;
    const int64_t ic = row / nBands;
    const int q = (int)(row - ic * nBands);
    const int64_t i = ic / nchOut;
    const BandItem it = items[i];
    const int c = it.nch == 2 ? (int)(ic - i * nchOut) : 0;
    double acc = 0.0;
    if (it.nTiles > 0) {
        // the frame in doubled samples, its ends clamped to the item's tiles first (lo <= every edge / 2 <= hi)
        const int64_t s = it.start + j * hop;                        // (start + nFrames hop was checked to fit)
        const int64_t s2 = 2 * min(max(s, (int64_t)it.lo), (int64_t)it.hi), e2 = 2 * min(max(s + hop, (int64_t)it.lo), (int64_t)it.hi);
        const long long* E = edges + it.edge0;
        int a = 0, b = it.nTiles;                                    // the first tile with E[t + 1] > s2, or nTiles
        while (a < b) {
            const int m = (a + b) >> 1;
            if (E[m + 1] > s2) b = m;
            else a = m + 1;
        }
        const double* B = bandSums + (it.row0 + c) * nBands + q;
        for (int tl = a; tl < it.nTiles && E[tl] < e2; ++tl) {
            const int64_t ov2 = min((int64_t)E[tl + 1], e2) - max((int64_t)E[tl], s2);
            if (ov2 > 0) acc += (double)ov2 * B[(int64_t)tl * it.nch * nBands];
        }
    }
    if (format == MRC_WINDOW_F64) ((double*)out)[o] = acc;
    else ((float*)out)[o] = (float)acc;
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

hipError_t launch_resample_out(int64_t nItems, const WindowItem* items, const long long* outStart, int64_t window, int nchOut,
                               int format, int L, int64_t planeLen, int up, int down, int W, int evenOdd, int skew,
                               const double* taps, const double* planes, void* out, hipStream_t st) {
    if (nItems <= 0 || window <= 0) return hipSuccess;
    const int64_t tiles = (window + kResampleThreads - 1) / kResampleThreads;
    const int64_t blocks = tiles * nItems * nchOut;
    if (blocks > 0x7fffffffLL || up < 1 || down < 1 || W < 1 ||
        ((int64_t)(kResampleThreads - 1) * down + up - 1) / up + 2 * (int64_t)W + 1 > kResampleRun)
        return hipErrorInvalidValue;                                 // (a run that would not fit the workgroup's LDS)
    hipLaunchKernelGGL(resample_out_kernel, dim3((unsigned)blocks), dim3(kResampleThreads), 0, st, items, outStart, window, tiles,
                       nchOut, format, L, planeLen, up, down, W, evenOdd, skew, taps, planes, out);
    return hipGetLastError();
}

hipError_t launch_sum_out(int64_t nRows, const SumTerm* terms, const long long* termOffset, int64_t window, int nchOut,
                          int format, int L, const double* planes, void* out, hipStream_t st) {
    if (nRows <= 0 || window <= 0) return hipSuccess;
    const int64_t tiles = (window + kWindowThreads - 1) / kWindowThreads;
    const int64_t blocks = tiles * nRows * nchOut;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;          // (the caller cuts such a call into slabs)
    hipLaunchKernelGGL(sum_out_kernel, dim3((unsigned)blocks), dim3(kWindowThreads), 0, st, terms, termOffset, window, tiles,
                       nchOut, format, L, planes, out);
    return hipGetLastError();
}

hipError_t launch_resample_sum_out(int64_t nRows, const SumTerm* terms, const long long* termOffset, int64_t window, int nchOut,
                                   int format, int L, int64_t planeLen, int up, int down, int W, int evenOdd, int skew,
                                   const double* taps, const double* planes, void* out, hipStream_t st) {
    if (nRows <= 0 || window <= 0) return hipSuccess;
    const int64_t tiles = (window + kResampleThreads - 1) / kResampleThreads;
    const int64_t blocks = tiles * nRows * nchOut;
    if (blocks > 0x7fffffffLL || up < 1 || down < 1 || W < 1 ||
        ((int64_t)(kResampleThreads - 1) * down + up - 1) / up + 2 * (int64_t)W + 1 > kResampleRun)
        return hipErrorInvalidValue;                                 // (a run that would not fit the workgroup's LDS)
    hipLaunchKernelGGL(resample_sum_out_kernel, dim3((unsigned)blocks), dim3(kResampleThreads), 0, st, terms, termOffset, window,
                       tiles, nchOut, format, L, planeLen, up, down, W, evenOdd, skew, taps, planes, out);
    return hipGetLastError();
}

hipError_t launch_resample_multi_sum_out(int64_t nRows, const SumTerm* terms, const int* ratioOf, const SpeedRatio* ratios,
                                         const SpeedRatio* ratiosHost, int nRatios, const long long* termOffset, int64_t window,
                                         int nchOut, int format, int L, int64_t planeLen, const double* planes, void* out,
                                         hipStream_t st) {
    if (nRows <= 0 || window <= 0) return hipSuccess;
    const int64_t tiles = (window + kResampleThreads - 1) / kResampleThreads;
    const int64_t blocks = tiles * nRows * nchOut;
    if (blocks > 0x7fffffffLL || nRatios < 1 || !ratiosHost) return hipErrorInvalidValue;
    for (int i = 0; i < nRatios; ++i) {
        const SpeedRatio& r = ratiosHost[i];
        if (r.W == 0) continue;                                      // the unit ratio: no run
        if (r.up < 1 || r.down < 1 || r.W < 1 || !r.taps ||
            ((int64_t)(kResampleThreads - 1) * r.down + r.up - 1) / r.up + 2 * (int64_t)r.W + 1 > kResampleRun)
            return hipErrorInvalidValue;                             // (a run that would not fit the workgroup's LDS)
    }
    hipLaunchKernelGGL(resample_multi_sum_out_kernel, dim3((unsigned)blocks), dim3(kResampleThreads), 0, st, terms, ratioOf, ratios,
                       termOffset, window, tiles, nchOut, format, L, planeLen, planes, out);
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

hipError_t launch_band_energy(const DevShape& F, int joint, int nBands, const int* lineLo, int64_t nEntries,
                              const EnergyEntry* entries, const int* oscale, const int* msSwitch, const int* scaleFactor,
                              const int* bitAlloc, const int* mantissa, double* bandSums, hipStream_t st) {
    if (nEntries <= 0) return hipSuccess;
    if (nBands < 1 || nBands > kBandThreads || nEntries > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(band_energy_kernel, dim3((unsigned)nEntries), dim3(kBandThreads), 0, st, F.bandOfLine, F.nBands, F.halfN,
                       F.nScaleBits, joint, nBands, lineLo, nEntries, entries, oscale, msSwitch, scaleFactor, bitAlloc, mantissa,
                       bandSums);
    return hipGetLastError();
}

hipError_t launch_filterbank_energy(const DevShape& F, int joint, int nFilters, const int* tab, const double* weight,
                                    int64_t nEntries, const EnergyEntry* entries, const int* oscale, const int* msSwitch,
                                    const int* scaleFactor, const int* bitAlloc, const int* mantissa, double* filterSums,
                                    hipStream_t st) {
    if (nEntries <= 0) return hipSuccess;
    if (nFilters < 1 || nFilters > kBandThreads || nEntries > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filterbank_energy_kernel, dim3((unsigned)nEntries), dim3(kBandThreads), 0, st, F.bandOfLine, F.nBands,
                       F.halfN, F.nScaleBits, joint, nFilters, tab, weight, nEntries, entries, oscale, msSwitch, scaleFactor,
                       bitAlloc, mantissa, filterSums);
    return hipGetLastError();
}

hipError_t launch_band_frames(int64_t nItems, const BandItem* items, const long long* edges, int64_t nFrames, int64_t hop,
                              int nBands, int nchOut, int format, const double* bandSums, void* out, hipStream_t st) {
    if (nItems <= 0 || nFrames <= 0) return hipSuccess;
    const int64_t total = nItems * nchOut * nBands * nFrames, blocks = (total + kFrameThreads - 1) / kFrameThreads;
    if (blocks > 0x7fffffffLL || (format != MRC_WINDOW_F32 && format != MRC_WINDOW_F64)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(band_frames_kernel, dim3((unsigned)blocks), dim3(kFrameThreads), 0, st, items, edges, total, nFrames, hop,
                       nBands, nchOut, format, bandSums, out);
    return hipGetLastError();
}

}  // namespace mrc
