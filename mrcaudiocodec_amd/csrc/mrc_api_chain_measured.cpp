// C ABI, the chained calls that measure their own output (include/mrc_hip.h): mrc_encode_chained_target_nmr_pac,
// mrc_encode_vbr_nmr_pac, mrc_encode_vbr_size_pac and their device entry points.  Each is a chained call (mrc_api_chain.cpp:
// chained_slabs, chained_core) with one ChainMeasure (mrc_chain_call.hpp) that says what its slabs do beside encoding.
//
//   source_analysis   once per slab, while its planes are in device memory: launch_nmr_source -- mrc_pac_nmr's own source
//                     analysis, mono, explicit offsets, thresholds written, MRC_OPT_EXACT_SPREAD honoured -- on the streams'
//                     own rows and on Close()'s gathered blocks, in batches of kTargetBatch blocks of one shape, each batch
//                     handed to the call's consumer kernel: nmr_rungs_kernel (the rungs of a ladder, behind the pack),
//                     vbr_alloc_kernel or vbr_profile_kernel (in place of the serial scan).
//                     (The analysis is run again rather than taken from phase A's lines: a joint group keeps L, R, M, S rows
//                     of one block side by side and comes from the four-signal kernels, mrc_pac_nmr's X from the one-signal
//                     kernels on explicit offsets; the numbers must be mrc_pac_nmr's to the bit, so the call is its call.)
//   reduce_files      once the streams of a slab -- a stream cut into time slabs: its last slab -- have all their entries in
//                     TargetBufs::stat: nmr_file_kernel over [rungs x streams] pseudo-files, one small copy back, the dB
//                     values from nmr_file_values on the host.
//
// Encode to a target noise-to-mask ratio: a rate ladder whose rungs are measured where they are made; target_decide applies
// the rule and gathers the chosen files behind each other in TargetBufs::sel, and the caller's buffer receives that run alone.
// Constant-quality VBR (the rule: DESIGN.md section 12): a one-rate call without a budget; phase A stops at the M/S switch,
// vbr_alloc_kernel writes the planes the packer reads, the entries' statistics and the capped bands, the packer chooses the
// Huffman tables, the bytes travel as the one-rate chained call's do.  VBR to a file size: the same
// slab with vbr_profile_kernel in vbr_alloc_kernel's place and VbrMeasure::search behind it; everything after it is the VBR call's.
#include "mrc_chain_call.hpp"

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

using namespace mrc;

namespace {

constexpr int64_t kTargetBatch = 16384;   // blocks of one shape analysed at a time: X and T of a batch stay below 512 MB

int64_t stream_chunks(const ChainCall& c, const int64_t* block_start, int64_t s) {   // blocks + Close(), a chunk per channel
    return c.nch() * (block_start[s + 1] - block_start[s] + 1);
}

// chunks of one rung of the streams that are decided together with the slab of the slab's call c
int64_t unit_chunks(const ChainCall& c, const ChainMeasure& N) {
    return c.slab->timeSlab ? stream_chunks(c, N.blockStart, c.slab->s0) : c.n_chunks();
}

// One batch of the source analysis: n blocks of group g (shape S; joint: two output channels), the first of them the
// group's k0-th; X and T hold the lines and thresholds [channel][n][halfN]; chunkBase: the entries of a time slab behind its
// stream's first start there in the stream's rows of TargetBufs::stat.
using SourceConsumer = std::function<int(int g, const DevShape& S, int joint, int64_t n, int64_t k0, const double* X,
                                         const double* T, int64_t chunkBase)>;

// The source analysis of a slab's call c: the rows of `stat` ([rungs][unitChunks][2]) reserved with the first slab of the
// streams decided together, the batch buffers sized, Close()'s offsets uploaded, `started` (if any) recorded, then every
// batch analysed and consumed.
int source_analysis(mrc_handle* h, const ChainCall& c, ChainMeasure& N, const ChainSchedule& q, const int64_t* count, int rungs,
                    hipEvent_t started, hipStream_t st, const SourceConsumer& consume) {
    ChainBufs& C = h->chain;
    TargetBufs& T = h->target;
    const Slab& sl = *c.slab;
    const int nch = c.nch(), L = h->cfg.n_mdct_lines;
    int64_t chunkBase = 0;
    if (sl.first) {
        N.unitChunks = unit_chunks(c, N);
        MRC_HIP(h, T.stat.reserve((size_t)(rungs * N.unitChunks) * 2 * sizeof(double)));
    } else chunkBase = nch * (sl.i0 - N.blockStart[sl.s0]);
    size_t rowBytes = 0, rows = 0;
    for (int g = 0; g < q.nGroups; ++g) {
        const int nOut = (g == 4 || nch == 1) ? 1 : 2;
        const size_t n = (size_t)std::min<int64_t>(count[g], kTargetBatch) * nOut;
        rows = std::max(rows, n);
        rowBytes = std::max(rowBytes, n * q.hs[g]->dev.halfN * sizeof(double));
    }
    MRC_HIP(h, T.lines.reserve(std::max<size_t>(rowBytes, 256)));
    MRC_HIP(h, T.thresh.reserve(std::max<size_t>(rowBytes, 256)));
    MRC_HIP(h, T.oscale.reserve(std::max<size_t>(rows * sizeof(int), 256)));
    MRC_HIP(h, T.smr.reserve(std::max<size_t>(rows * kMaxBands * sizeof(double), 256)));
    if (c.with_flush) {
        N.flushOffs.resize((size_t)count[4]);
        for (int64_t k = 0; k < count[4]; ++k) N.flushOffs[(size_t)k] = k * 2 * (int64_t)L;
        MRC_HIP(h, T.flushOffs.reserve(std::max<size_t>(N.flushOffs.size() * sizeof(int64_t), 256)));
        if (count[4])
            MRC_HIP(h, hipMemcpyAsync(T.flushOffs.p, N.flushOffs.data(), N.flushOffs.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    }
    if (started) MRC_HIP(h, hipEventRecord(started, st));
    for (int g = 0; g < q.nGroups; ++g) {
        if (!count[g]) continue;
        const DevShape& S = q.hs[g]->dev;
        const int joint = (g == 4 || nch == 1) ? 0 : 1, nOut = joint ? 2 : 1, M = S.halfN;
        for (int64_t k0 = 0; k0 < count[g]; k0 += kTargetBatch) {
            const int64_t n = std::min<int64_t>(kTargetBatch, count[g] - k0);
            const int64_t* offs = (g == 4 ? T.flushOffs.as<int64_t>() : C.g[g].offsets.as<int64_t>()) + k0;
            for (int ch = 0; ch < nOut; ++ch) {
                const void* src = g == 4 ? C.flushPcm.p : (ch ? c.pcm_right : c.pcm_left);
                MRC_HIP(h, launch_nmr_source(h, S, n, src, offs, T.lines.as<double>() + ch * n * M, T.oscale.as<int>() + ch * n,
                                             T.smr.as<double>() + ch * n * kMaxBands, T.thresh.as<double>() + ch * n * M, st));
            }
            MRC_TRY(consume(g, S, joint, n, k0, T.lines.as<double>(), T.thresh.as<double>(), chunkBase));
        }
    }
    return MRC_OK;
}

// The streams sl.s0 .. sl.s0 + sl.ns - 1 have all their entries in stat, `rungs` rows of N.unitChunks: pseudo-file (r, s) is
// the entries [r * unitChunks + first chunk of s, ...) in file order.  -> start [ns + 1]: the first chunk of every stream
// inside a row; fileOut [rungs * ns][4]: nmr_file_kernel's sums.  ev (if any): recorded around the kernel.  Synchronises.
int reduce_files(mrc_handle* h, const ChainCall& c, const ChainMeasure& N, const Slab& sl, int rungs, const Event* ev,
                 hipStream_t st, std::vector<long long>* start, std::vector<double>* fileOut) {
    TargetBufs& T = h->target;
    const int64_t ns = sl.ns, nFiles = rungs * ns;
    start->assign((size_t)ns + 1, 0);
    for (int64_t s = 0; s < ns; ++s) (*start)[(size_t)s + 1] = (*start)[(size_t)s] + stream_chunks(c, N.blockStart, sl.s0 + s);
    std::vector<long long> tab((size_t)nFiles + 1 + (size_t)(nFiles + 1) / 2 + 1);   // starts [nFiles + 1], then nch [nFiles] packed
    int* nchTab = (int*)(tab.data() + nFiles + 1);
    for (int r = 0; r < rungs; ++r)
        for (int64_t s = 0; s < ns; ++s) {
            tab[(size_t)(r * ns + s)] = r * N.unitChunks + (*start)[(size_t)s];
            nchTab[r * ns + s] = c.nch();
        }
    tab[(size_t)nFiles] = rungs * N.unitChunks;
    fileOut->assign((size_t)nFiles * 4, 0.0);
    MRC_HIP(h, T.fileTab.reserve(tab.size() * sizeof(long long)));
    MRC_HIP(h, T.fileOut.reserve(fileOut->size() * sizeof(double)));
    DrainGuard guard{{st}};                              // (behind the vectors queued copies read and write)
    MRC_HIP(h, hipMemcpyAsync(T.fileTab.p, tab.data(), tab.size() * sizeof(long long), hipMemcpyHostToDevice, st));
    if (ev) MRC_HIP(h, hipEventRecord(ev[0], st));
    MRC_HIP(h, launch_nmr_file(nFiles, T.fileTab.as<long long>(), (const int*)(T.fileTab.as<long long>() + nFiles + 1),
                               T.stat.as<double>(), T.fileOut.as<double>(), st));
    if (ev) MRC_HIP(h, hipEventRecord(ev[1], st));
    MRC_HIP(h, hipMemcpyAsync(fileOut->data(), T.fileOut.p, fileOut->size() * sizeof(double), hipMemcpyDeviceToHost, st));
    MRC_HIP(h, hipStreamSynchronize(st));
    return MRC_OK;
}

// the weight of stream gs of the caller's call c in its file's mean (the sum of b over blocks and channels, Close()'s block
// included) and its number of blocks
int64_t stream_weight(mrc_handle* h, const ChainCall& c, int64_t gs, int64_t* n_blocks) {
    int64_t weight = (int64_t)h->cfg.n_mdct_lines * c.nch();                    // Close()'s block
    for (int64_t i = c.block_start[gs]; i < c.block_start[gs + 1]; ++i) weight += (int64_t)c.block_b[i] * c.nch();
    *n_blocks = c.block_start[gs + 1] - c.block_start[gs] + 1;
    return weight;
}

// ---- the refusals of include/mrc_hip.h that these calls share, before any device work

// the block layout a call that measures its own output needs (the NMR positions blocks by their offsets; whole files)
int layout_check(mrc_handle* h, const std::string& w, const ChainCall& c) {
    const int L = h->cfg.n_mdct_lines;
    for (int64_t s = 0; s < c.n_streams; ++s) {
        const int64_t i0 = c.block_start[s], i1 = c.block_start[s + 1];
        const std::string which = w + ": stream " + std::to_string(s);
        if (i1 <= i0) return fail(h, MRC_ERR_INVALID, which + ": block_start gives it no block");
        if (c.block_a[i0] != L)
            return fail(h, MRC_ERR_INVALID, which + ": block_a of its first block must be n_mdct_lines (the zero prior hop)");
        int64_t sum = 0;
        for (int64_t i = i0; i < i1; ++i) {
            if (c.block_offset[i] != sum)
                return fail(h, MRC_ERR_INVALID, which + ": block_offset[" + std::to_string(i) + "] must be the sum of block_a of the "
                                                "stream's earlier blocks (" + std::to_string(sum) + "): the NMR positions blocks by it");
            sum += c.block_a[i];
        }
        if (c.block_b[i1 - 1] != L)
            return fail(h, MRC_ERR_INVALID, which + ": block_b of its last block must be n_mdct_lines (a stream must end with a long "
                                            "block: the reference's Close() assumes it, pacfileThem.py:973-984)");
    }
    return MRC_OK;
}

// whole files only, no certificate (sensWhy: why not), no NULL among the common arguments (results: nor among the call's
// own), the layout
int whole_files_check(mrc_handle* h, const std::string& w, const ChainCall& c, const char* sensWhy, const uint8_t* out,
                      int64_t out_cap, bool results) {
    if (!c.num_samples) return fail(h, MRC_ERR_INVALID, w + ": num_samples must not be NULL (whole files only)");
    if (h->sensOn) return fail(h, MRC_ERR_INVALID, w + ": MRC_OPT_SENSITIVITY is on (" + sensWhy + ")");
    if (c.n_streams < 0 || !c.pcm_left || c.stream_stride <= 0 || !c.block_start || !c.block_offset || !c.block_a || !c.block_b ||
        !out || out_cap < 0 || !results)
        return fail(h, MRC_ERR_INVALID, w + ": bad argument (a NULL pointer, a negative count or capacity)");
    return layout_check(h, w, c);
}

// ---- encode to a target noise-to-mask ratio

struct TargetSeg { int r; int64_t off, n; };   // bytes of rung r of one time slab in TargetBufs::keep

// every slab measures its rungs behind the pack
struct TargetMeasure : ChainMeasure {
    std::vector<TargetSeg> segs;
    int64_t keepUsed = 0, selUsed = 0;
    double msGather = 0;
    int behind_pack(mrc_handle* h, const ChainCall& c, const ChainSchedule& q, const int64_t* count, hipStream_t st) override {
        ChainBufs& C = h->chain;
        TargetBufs& T = h->target;
        MRC_TRY(source_analysis(h, c, *this, q, count, c.n_rates, T.ev[0], st,
            [&](int g, const DevShape& S, int joint, int64_t n, int64_t k0, const double* X, const double* Th, int64_t chunkBase) {
                MRC_HIP(h, launch_nmr_rungs(S, c.n_rates, joint, n, k0, C.groupDesc.as<ChainGroupDev>(), g,
                                            C.g[g].chunkMap.as<long long>() + k0 * (joint ? 2 : 1), X, Th, T.stat.as<double>(),
                                            unitChunks, chunkBase, st));
                return (int)MRC_OK;
            }));
        MRC_HIP(h, hipEventRecord(T.ev[1], st));
        return MRC_OK;
    }
    int read_events(mrc_handle* h) override {
        double ms = 0;
        MRC_HIP(h, h->target.ev.elapsed(0, 1, &ms));
        msMeasure += ms;
        return MRC_OK;
    }
};

// room for `need` more bytes behind the `used` bytes a buffer holds, which stay
int grow_kept(mrc_handle* h, DevBuf& b, int64_t used, int64_t need, hipStream_t st) {
    if ((size_t)(used + need) <= b.cap) return MRC_OK;
    DevBuf bigger;
    MRC_HIP(h, bigger.reserve(std::max<size_t>(2 * b.cap, (size_t)(used + need))));
    hipError_t e = hipSuccess;
    if (used) e = hipMemcpyAsync(bigger.p, b.p, (size_t)used, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(h, e, "mrc_encode_chained_target_nmr_pac: growing a device buffer");
    b = std::move(bigger);                               // (which leaves with b's old allocation and frees it)
    return MRC_OK;
}

// what a call returns beside the bytes
struct TargetOut {
    double target;
    int64_t* stream_byte_offset; int32_t *chosen, *met;
    double *nmr_total_db, *nmr_max_db; int64_t *disturbed_blocks, *n_blocks;
};

// The streams of slab sl have all their entries in stat and all their bytes packed: reduce, decide, gather.
// Whole-stream slab: rung r's bytes of stream s are at buf + base[r] + sOff[r][s]; time slabs: in the segments of `keep`.
int target_decide(mrc_handle* h, const ChainCall& c, TargetMeasure& N, const TargetOut& o, const Slab& sl, const int64_t* sOff,
                  const int64_t* base, const uint8_t* buf, hipStream_t st) {
    TargetBufs& T = h->target;
    const int R = c.n_rates;
    const int64_t nS = c.n_streams, ns = sl.ns;
    std::vector<long long> start, span((size_t)ns * 3);
    std::vector<double> fileOut;
    MRC_TRY(reduce_files(h, c, N, sl, R, &T.ev.ev[2], st, &start, &fileOut));
    // ---- the rule
    int64_t maxLen = 0, selNeed = 0;
    for (int64_t s = 0; s < ns; ++s) {
        const int64_t gs = sl.s0 + s;
        const int64_t weight = stream_weight(h, c, gs, &o.n_blocks[gs]);
        int pick = R - 1, met = 0;
        for (int r = R - 1; r >= 0; --r) {
            const NmrFileValues v = nmr_file_values(fileOut.data() + 4 * (r * ns + s), weight);
            o.nmr_max_db[r * nS + gs] = v.nmr_max_db;
            o.nmr_total_db[r * nS + gs] = v.nmr_total_db;
            o.disturbed_blocks[r * nS + gs] = v.disturbed_blocks;
            if (v.nmr_total_db <= o.target) { pick = r; met = 1; }              // (descending: the smallest r that meets it stays)
        }
        o.chosen[gs] = pick;
        o.met[gs] = met;
        o.stream_byte_offset[gs] = N.selUsed + selNeed;
        if (!sl.timeSlab) {
            const int64_t* so = sOff + pick * (ns + 1);
            span[(size_t)(3 * s)] = base[pick] + so[s];
            span[(size_t)(3 * s + 1)] = N.selUsed + selNeed;
            span[(size_t)(3 * s + 2)] = so[s + 1] - so[s];
            maxLen = std::max<int64_t>(maxLen, so[s + 1] - so[s]);
            selNeed += so[s + 1] - so[s];
        } else
            for (const TargetSeg& g : N.segs) if (g.r == pick) selNeed += g.n;
    }
    // ---- the chosen files behind each other
    MRC_TRY(grow_kept(h, T.sel, N.selUsed, std::max<int64_t>(selNeed, 1), st));
    DrainGuard guard{{st}};                              // (behind span, which a queued copy reads)
    MRC_HIP(h, hipEventRecord(T.ev[4], st));
    if (!sl.timeSlab) {
        MRC_HIP(h, T.span.reserve(span.size() * sizeof(long long)));
        MRC_HIP(h, hipMemcpyAsync(T.span.p, span.data(), span.size() * sizeof(long long), hipMemcpyHostToDevice, st));
        MRC_HIP(h, launch_target_gather(ns, maxLen, T.span.as<long long>(), buf, T.sel.as<unsigned char>(), st));
    } else {
        int64_t at = N.selUsed;
        for (const TargetSeg& g : N.segs)
            if (g.r == o.chosen[sl.s0] && g.n) {
                MRC_HIP(h, hipMemcpyAsync(T.sel.as<uint8_t>() + at, T.keep.as<uint8_t>() + g.off, (size_t)g.n, hipMemcpyDeviceToDevice, st));
                at += g.n;
            }
        N.segs.clear();
        N.keepUsed = 0;
    }
    MRC_HIP(h, hipEventRecord(T.ev[5], st));
    MRC_HIP(h, hipStreamSynchronize(st));
    N.selUsed += selNeed;
    double a = 0, b = 0;
    MRC_HIP(h, T.ev.elapsed(2, 3, &a));
    MRC_HIP(h, T.ev.elapsed(4, 5, &b));
    N.msMeasure += a;
    N.msGather += b;
    return MRC_OK;
}

int target_check(mrc_handle* h, const std::string& w, const ChainCall& c, const TargetOut& o, const uint8_t* out, int64_t out_cap,
                 const int64_t* total_bytes) {
    if (!h) return MRC_ERR_INVALID;
    MRC_TRY(rate_count_check(h, w, c.n_rates));
    if (!c.rates) return fail(h, MRC_ERR_INVALID, w + ": target_bits_per_sample must not be NULL");
    for (int r = 0; r < c.n_rates; ++r) MRC_TRY(rate_check(h, w, c.rates, r, true));
    if (std::isnan(o.target)) return fail(h, MRC_ERR_INVALID, w + ": target_nmr_total_db is NaN");
    return whole_files_check(h, w, c, "the certificate covers one rate: encode each rate on its own", out, out_cap,
                             o.stream_byte_offset && o.chosen && o.met && o.nmr_total_db && o.nmr_max_db && o.disturbed_blocks &&
                                 o.n_blocks && total_bytes);
}

// Both entry points: pcm and out in host memory (the PCM staged) or on the device.  The chosen bytes end in TargetBufs::sel
// and, if they fit, in out.
int target_call(mrc_handle* h, const std::string& w, ChainCall c, const TargetOut& o, uint8_t* out, int64_t out_cap,
                int64_t* total_bytes, bool onHost) {
    MRC_TRY(target_check(h, w, c, o, out, out_cap, total_bytes));
    forget_held_output(h);
    MRC_HIP(h, hipSetDevice(h->device));
    if (onHost) {
        MRC_TRY(stage_pcm(h, c));
        c.pcm_left = h->chain.pcmL.p;
        if (c.pcm_right) c.pcm_right = h->chain.pcmR.p;
    }
    hipStream_t st = onHost ? h->stream : pick_stream(h, c.stream);
    const int R = c.n_rates;
    const int64_t nS = c.n_streams;
    ChainBufs& C = h->chain;
    TargetBufs& T = h->target;
    MRC_HIP(h, T.ev.create());
    TargetMeasure N;
    N.blockStart = c.block_start;
    std::vector<int64_t> sOff((size_t)R * (nS + 1)), totals((size_t)R), caps((size_t)R, std::numeric_limits<int64_t>::max() / 4);
    c.stream_byte_offset = sOff.data();
    c.total_bytes = totals.data();
    c.measure = &N;
    *total_bytes = 0;
    o.stream_byte_offset[0] = 0;
    int rc = chained_slabs(h, c, caps.data(), nullptr,
        [&](const Slab& sl, int r, uint8_t* buf, int64_t n, int64_t) {
            if (!sl.timeSlab) return (int)MRC_OK;                    // (whole streams: gathered from the slab's buffer)
            MRC_TRY(grow_kept(h, T.keep, N.keepUsed, std::max<int64_t>(n, 1), st));
            if (n) MRC_HIP(h, hipMemcpyAsync(T.keep.as<uint8_t>() + N.keepUsed, buf, (size_t)n, hipMemcpyDeviceToDevice, st));
            N.segs.push_back(TargetSeg{r, N.keepUsed, n});
            N.keepUsed += n;
            return (int)MRC_OK;
        },
        [&](const Slab& sl, const int64_t* slabOff, const int64_t* base, const uint8_t* buf) {
            if (sl.last) MRC_TRY(target_decide(h, c, N, o, sl, slabOff, base, buf, st));
            return (int)MRC_OK;
        });
    T.ms[0] = h->chainMs[0]; T.ms[1] = h->chainMs[1]; T.ms[2] = N.msMeasure; T.ms[3] = h->chainMs[2] + N.msGather;
    if (rc != MRC_OK) return rc;
    const int64_t total = N.selUsed;
    *total_bytes = total;
    o.stream_byte_offset[nS] = total;
    C.lastTotal = total;                                 // (mrc_chain_fetch_output: the chosen bytes, whatever out_cap was)
    C.lastSrc = T.sel.p;
    if (total > out_cap) return fail(h, MRC_ERR_NOMEM, w + ": out_cap too small (see total_bytes; mrc_chain_fetch_output)");
    if (total) MRC_HIP(h, hipMemcpyAsync(out, T.sel.p, (size_t)total, onHost ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
    MRC_HIP(h, hipStreamSynchronize(st));
    return MRC_OK;
}

// ---- constant-quality VBR, and VBR to a file size

// mrc_encode_vbr_size_pac: the grid, the size limits and the per-stream results of the search, all the caller's
struct VbrSize {
    double lo, step; int n; const int64_t* target;
    int32_t* chosen; double *chosen_db, *ceiling_ratio; int32_t *met, *probes, *probe_index; int64_t* probe_bytes;
    double db(int i) const { return lo + (double)i * step; }
};

struct VbrOut { int64_t *capped_bands, *coded_bits; double *nmr_total_db, *nmr_max_db; int64_t *disturbed_blocks, *n_blocks; };

// no budget, no scan: every slab allocates per band against measured noise (msMeasure: the allocator or the recorder alone)
struct VbrMeasure : ChainMeasure {
    double ceiling = 0.0;            // c, the linear ratio
    const VbrSize* size = nullptr;   // mrc_encode_vbr_size_pac: the slab records the walk and searches the grid (search)
    double msProbe = 0, msPick = 0;
    bool allocates() const override { return true; }
    int in_place_of_scan(mrc_handle* h, const ChainCall& c, const ChainSchedule& q, const int64_t* count, hipStream_t st) override;
    int search(mrc_handle* h, const ChainCall& c, const ChainSchedule& q, const int64_t* count, hipStream_t st);
    int read_events(mrc_handle* h) override;
};

// The search of one slab's streams (include/mrc_hip.h states the rule): the record of every block is in VbrBufs::prof.  A
// probe: vbr_pick_kernel at each stream's ceiling, the packer's plan (pricing only), the streams' file sizes, one copy back;
// the host moves every unfinished stream's interval.  At most MRC_MAX_PROBES rounds whatever the number of streams.  It
// leaves the planes, T.stat and V.capped at the chosen ceilings, as vbr_alloc_kernel would.
int VbrMeasure::search(mrc_handle* h, const ChainCall& c, const ChainSchedule& q, const int64_t* count, hipStream_t st) {
    const VbrSize& Z = *size;
    ChainBufs& C = h->chain;
    TargetBufs& T = h->target;
    VbrBufs& V = h->vbr;
    const int nch = c.nch();
    const int64_t nS = c.n_streams, nChunks = c.n_chunks(), s0 = c.slab->s0;
    MRC_HIP(h, V.ceilings.reserve((size_t)nS * sizeof(double)));
    MRC_HIP(h, V.bytes.reserve((size_t)nS * sizeof(long long)));
    MRC_HIP(h, C.packWs.reserve(pack_workspace_bytes(nChunks)));
    const PackWs W = pack_ws_views(C.packWs.p, nChunks);
    const PackTables& tables = host_pack_tables();
    std::vector<int> lo((size_t)nS, 0), hi((size_t)nS, Z.n - 1), at((size_t)nS, -1);
    std::vector<char> active((size_t)nS, 1);
    std::vector<double> ceil((size_t)nS);
    std::vector<long long> bytes((size_t)nS);
    auto pick = [&]() -> int {                           // every block at the ceiling at[] of its stream
        for (int64_t s = 0; s < nS; ++s) ceil[(size_t)s] = std::pow(10.0, Z.db(at[(size_t)s]) / 10.0);
        MRC_HIP(h, hipMemcpyAsync(V.ceilings.p, ceil.data(), (size_t)nS * sizeof(double), hipMemcpyHostToDevice, st));
        for (int g = 0; g < q.nGroups; ++g) {
            const int joint = (g == 4 || nch == 1) ? 0 : 1;
            ChainGroupBufs& B = C.g[g];
            MRC_HIP(h, launch_vbr_pick(q.hs[g]->dev, joint, count[g], V.ceilings.as<double>(), C.chunkStream.as<int>(),
                                       B.lines.as<double>(), B.oscale.as<int>(), joint ? B.ms.as<int>() : nullptr,
                                       V.prof[g].as<double>(), joint ? V.profPick[g].as<unsigned>() : nullptr,
                                       B.bitAlloc.as<int>(), B.scaleFactor.as<int>(), B.mant.as<unsigned short>(),
                                       B.chunkMap.as<long long>(), T.stat.as<double>(), V.capped.as<int>(), st));
        }
        return MRC_OK;
    };
    MRC_HIP(h, hipEventRecord(V.evSize[0], st));
    for (int round = 0; round < MRC_MAX_PROBES; ++round) {
        bool any = false;
        for (int64_t s = 0; s < nS; ++s)
            if (active[(size_t)s]) { at[(size_t)s] = round == 0 ? hi[(size_t)s] : (lo[(size_t)s] + hi[(size_t)s]) / 2; any = true; }
        if (!any) break;
        MRC_TRY(pick());
        for (int g = 0; g < q.nGroups; ++g) {
            if (!count[g]) continue;
            const int joint = (g == 4 || nch == 1) ? 0 : 1;
            const DevShape& S = q.hs[g]->dev;
            ChainGroupBufs& B = C.g[g];
            MRC_HIP(h, launch_pack_plan(S, pack_params(h->cfg, S.a, S.b, joint ? 2 : 1, joint, c.use_huffman), tables, count[g],
                                        B.bitAlloc.as<int>(), B.mant.as<unsigned short>(), MRC_MANTISSA_I16, nullptr,
                                        B.table.as<int>(), nullptr, W, B.chunkMap.as<long long>(), all_bands_non_empty(*q.hs[g]), st));
        }
        MRC_HIP(h, launch_vbr_size_bytes(nS, nChunks, q.hdrLen, C.firstChunk.as<long long>(), W.chunkBytes, V.bytes.as<long long>(), st));
        MRC_HIP(h, hipMemcpyAsync(bytes.data(), V.bytes.p, (size_t)nS * sizeof(long long), hipMemcpyDeviceToHost, st));
        MRC_HIP(h, hipStreamSynchronize(st));
        for (int64_t s = 0; s < nS; ++s) {
            if (!active[(size_t)s]) continue;
            const int64_t gs = s0 + s;
            const int i = at[(size_t)s], p = Z.probes[gs]++;
            const bool fits = bytes[(size_t)s] <= Z.target[gs];
            if (Z.probe_index) Z.probe_index[gs * MRC_MAX_PROBES + p] = i;
            if (Z.probe_bytes) Z.probe_bytes[gs * MRC_MAX_PROBES + p] = bytes[(size_t)s];
            if (round == 0) {
                Z.met[gs] = fits ? 1 : 0;
                if (!fits) active[(size_t)s] = 0;
            } else if (fits) hi[(size_t)s] = i;
            else lo[(size_t)s] = i + 1;
            if (lo[(size_t)s] >= hi[(size_t)s]) active[(size_t)s] = 0;
        }
    }
    MRC_HIP(h, hipEventRecord(V.evSize[1], st));
    bool again = false;
    for (int64_t s = 0; s < nS; ++s) {
        const int64_t gs = s0 + s;
        again = again || at[(size_t)s] != hi[(size_t)s];
        at[(size_t)s] = hi[(size_t)s];
        Z.chosen[gs] = hi[(size_t)s];
        Z.chosen_db[gs] = Z.db(hi[(size_t)s]);
        Z.ceiling_ratio[gs] = std::pow(10.0, Z.chosen_db[gs] / 10.0);
    }
    if (again) MRC_TRY(pick());
    MRC_HIP(h, hipEventRecord(V.evSize[2], st));
    MRC_HIP(h, hipStreamSynchronize(st));                // (the queued copy reads ceil)
    return MRC_OK;
}

// where the serial scan would run: the source analysis, every batch consumed by vbr_alloc_kernel -- or recorded by
// vbr_profile_kernel, and the search behind the last batch -- between an event pair of its own
int VbrMeasure::in_place_of_scan(mrc_handle* h, const ChainCall& c, const ChainSchedule& q, const int64_t* count, hipStream_t st) {
    ChainBufs& C = h->chain;
    TargetBufs& T = h->target;
    VbrBufs& V = h->vbr;
    const int nch = c.nch();
    if (c.slab->first) MRC_HIP(h, V.capped.reserve((size_t)unit_chunks(c, *this) * sizeof(int)));
    size_t launches = 0;
    for (int g = 0; g < q.nGroups; ++g) launches += (size_t)((count[g] + kTargetBatch - 1) / kTargetBatch);
    while (V.ev.size() < 2 * launches) {
        Event e;
        MRC_HIP(h, e.create());
        V.ev.push_back(std::move(e));
    }
    V.evUsed = 0;
    if (size) {                                          // the record of every block of the slab, group by group
        MRC_HIP(h, V.evSize.create());
        for (int g = 0; g < q.nGroups; ++g) {
            const int joint = (g == 4 || nch == 1) ? 0 : 1;
            MRC_HIP(h, V.prof[g].reserve(std::max<size_t>((size_t)count[g] * vbr_profile_bytes(q.hs[g]->dev, joint), 256)));
            if (joint) MRC_HIP(h, V.profPick[g].reserve(std::max<size_t>((size_t)count[g] * q.hs[g]->dev.nBands * sizeof(unsigned), 256)));
        }
    }
    MRC_TRY(source_analysis(h, c, *this, q, count, 1, nullptr, st,
        [&](int g, const DevShape& S, int joint, int64_t n, int64_t k0, const double* X, const double* Th, int64_t chunkBase) {
            ChainGroupBufs& B = C.g[g];
            const int* ms = joint ? B.ms.as<int>() : nullptr;
            MRC_HIP(h, hipEventRecord(V.ev[V.evUsed++], st));
            if (size)
                MRC_HIP(h, launch_vbr_profile(S, joint, n, k0, B.lines.as<double>(), B.oscale.as<int>(), ms, X, Th,
                                              V.prof[g].as<double>(), joint ? V.profPick[g].as<unsigned>() : nullptr, st));
            else
                MRC_HIP(h, launch_vbr_alloc(S, joint, n, k0, ceiling, B.lines.as<double>(), B.oscale.as<int>(), ms,
                                            B.bitAlloc.as<int>(), B.scaleFactor.as<int>(), B.mant.as<unsigned short>(),
                                            B.chunkMap.as<long long>() + k0 * (joint ? 2 : 1), X, Th, T.stat.as<double>(),
                                            V.capped.as<int>(), chunkBase, st));
            MRC_HIP(h, hipEventRecord(V.ev[V.evUsed++], st));
            return (int)MRC_OK;
        }));
    if (size) MRC_TRY(search(h, c, q, count, st));
    return MRC_OK;
}

int VbrMeasure::read_events(mrc_handle* h) {
    VbrBufs& V = h->vbr;
    for (size_t i = 0; i + 1 < V.evUsed; i += 2) {
        double ms = 0;
        MRC_HIP(h, V.ev[i].ms_until(V.ev[i + 1], &ms));
        msMeasure += ms;
    }
    if (size) {
        double a = 0, b = 0;
        MRC_HIP(h, V.evSize.elapsed(0, 1, &a));
        MRC_HIP(h, V.evSize.elapsed(1, 2, &b));
        msProbe += a;
        msPick += b;
    }
    return MRC_OK;
}

// The streams of slab sl have all their entries in stat: the file reduction, the dB values, the capped bands.
int vbr_decide(mrc_handle* h, const ChainCall& c, const VbrMeasure& N, const VbrOut& o, const Slab& sl, hipStream_t st) {
    std::vector<long long> start;
    std::vector<double> fileOut;
    MRC_TRY(reduce_files(h, c, N, sl, 1, nullptr, st, &start, &fileOut));
    std::vector<int> capped((size_t)start.back());
    DrainGuard guard{{st}};                              // (behind the vector a queued copy writes)
    MRC_HIP(h, hipMemcpyAsync(capped.data(), h->vbr.capped.p, capped.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    MRC_HIP(h, hipStreamSynchronize(st));
    for (int64_t s = 0; s < sl.ns; ++s) {
        const int64_t gs = sl.s0 + s;
        const int64_t weight = stream_weight(h, c, gs, &o.n_blocks[gs]);
        const NmrFileValues v = nmr_file_values(fileOut.data() + 4 * s, weight);
        o.nmr_total_db[gs] = v.nmr_total_db;
        o.nmr_max_db[gs] = v.nmr_max_db;
        o.disturbed_blocks[gs] = v.disturbed_blocks;
        int64_t cap = 0;
        for (long long k = start[(size_t)s]; k < start[(size_t)s + 1]; ++k) cap += capped[(size_t)k];
        o.capped_bands[gs] = cap;
    }
    return MRC_OK;
}

// mrc_encode_vbr_size_pac's own refusals behind the common ones, and the trace cleared; cap: the blocks a slab of it holds
int vbr_size_check(mrc_handle* h, const std::string& w, const VbrSize& Z, const ChainCall& c, int64_t cap) {
    if (!std::isfinite(Z.lo)) return fail(h, MRC_ERR_INVALID, w + ": ceiling_lo_db must be finite");
    if (!std::isfinite(Z.step) || !(Z.step > 0.0)) return fail(h, MRC_ERR_INVALID, w + ": ceiling_step_db must be finite and > 0");
    if (Z.n < 1 || Z.n > MRC_MAX_CEILINGS) return fail(h, MRC_ERR_INVALID, w + ": n_ceilings must lie in 1..MRC_MAX_CEILINGS (256)");
    if (!Z.target) return fail(h, MRC_ERR_INVALID, w + ": target_bytes must not be NULL");
    if (!Z.chosen || !Z.chosen_db || !Z.met || !Z.probes)
        return fail(h, MRC_ERR_INVALID, w + ": chosen, chosen_db, met and probes must not be NULL");
    for (int64_t s = 0; s < c.n_streams; ++s) {
        const int64_t nb = c.block_start[s + 1] - c.block_start[s];
        if (Z.target[s] < 0) return fail(h, MRC_ERR_INVALID, w + ": target_bytes[" + std::to_string(s) + "] is negative");
        if (nb > cap)
            return fail(h, MRC_ERR_INVALID, w + ": stream " + std::to_string(s) + " has " + std::to_string(nb) +
                                            " blocks, a slab of this call holds " + std::to_string(cap) + " (MRC_OPT_CHAIN_SLAB_BLOCKS): "
                                            "the search needs all blocks of a stream resident at once");
    }
    for (int64_t s = 0; s < c.n_streams; ++s) {
        Z.probes[s] = 0;
        for (int p = 0; p < MRC_MAX_PROBES; ++p) {
            if (Z.probe_index) Z.probe_index[s * MRC_MAX_PROBES + p] = -1;
            if (Z.probe_bytes) Z.probe_bytes[s * MRC_MAX_PROBES + p] = -1;
        }
    }
    return MRC_OK;
}

// behind the slabs: the sizes as payload bits, the times
int vbr_finish(mrc_handle* h, const ChainCall& c, const VbrMeasure& N, const VbrOut& o) {
    uint8_t one[256];
    int64_t hdrLen = 0;
    if (c.n_streams && (mrc_pac_header(&h->cfg, c.nch(), c.num_samples[0], one, sizeof(one), &hdrLen) != MRC_OK))
        return fail(h, MRC_ERR_INVALID, "mrc_encode_vbr_nmr_pac: mrc_pac_header failed");
    for (int64_t s = 0; s < c.n_streams; ++s)            // a chunk: a 4-byte length and its payload
        o.coded_bits[s] = 8 * (c.stream_byte_offset[s + 1] - c.stream_byte_offset[s] - hdrLen - 4 * stream_chunks(c, c.block_start, s));
    VbrBufs& V = h->vbr;
    V.ms[0] = h->chainMs[0] + h->chainMs[1] - N.msMeasure;
    V.ms[1] = N.msMeasure;
    V.ms[2] = h->chainMs[2];
    V.ms[3] = h->chainMs[3];
    if (N.size) {
        V.sizeMs[0] = V.ms[0] - N.msProbe - N.msPick;
        V.sizeMs[1] = N.msMeasure;
        V.sizeMs[2] = N.msProbe;
        V.sizeMs[3] = N.msPick + h->chainMs[2];
        V.sizeMs[4] = h->chainMs[3];
    }
    return MRC_OK;
}

// All four entry points: one ceiling (Z == nullptr: ceiling_db, its ratio to *ceiling_ratio) or a search (Z); pcm and out in
// host memory (the PCM staged, the bytes copied back slab by slab) or on the device.
int vbr_call(mrc_handle* h, const std::string& w, double ceiling_db, const VbrSize* Z, ChainCall c, const VbrOut& o, uint8_t* out,
             int64_t out_cap, double* ceiling_ratio, bool onHost) {
    if (!h) return MRC_ERR_INVALID;
    if (std::isnan(ceiling_db)) return fail(h, MRC_ERR_INVALID, w + ": ceiling_db is NaN");
    MRC_TRY(whole_files_check(h, w, c, "the certificate covers the budgeted allocation, not this one", out, out_cap,
                              c.stream_byte_offset && ceiling_ratio && o.capped_bands && o.coded_bits && o.nmr_total_db &&
                                  o.nmr_max_db && o.disturbed_blocks && o.n_blocks && c.total_bytes));
    VbrMeasure N;
    N.blockStart = c.block_start;
    N.size = Z;
    if (Z) {
        c.slabBlocks = vbr_size_slab_blocks(h, c.nch());
        MRC_TRY(vbr_size_check(h, w, *Z, c, c.slabBlocks));
    } else N.ceiling = *ceiling_ratio = std::pow(10.0, ceiling_db / 10.0);
    c.measure = &N;
    hipStream_t st = onHost ? h->stream : pick_stream(h, c.stream);
    const ChainAfter after = [&](const Slab& sl, const int64_t*, const int64_t*, const uint8_t*) {
        if (sl.last) MRC_TRY(vbr_decide(h, c, N, o, sl, st));    // (a stream in time slabs: once its last slab ran)
        return (int)MRC_OK;
    };
    int rc;
    if (onHost) rc = chained_host(h, w.c_str(), c, &out, &out_cap, after);
    else {
        MRC_TRY(check_call(h, w.c_str(), c, &out, &out_cap));
        rc = chained_slabs(h, c, &out_cap, out, {}, after);
    }
    if (rc != MRC_OK && rc != MRC_ERR_NOMEM) return rc;
    const std::string err = h->error;                    // (a buffer too small: the numbers are complete all the same)
    MRC_TRY(vbr_finish(h, c, N, o));
    if (rc != MRC_OK) h->error = err;
    return rc;
}

// The stage entries of the VBR kernels (mrc_dev_vbr_alloc, _profile, _pick): n independent blocks of one shape on the caller's
// planes.  File order as the launches take it: the chunks of block k are ns k, ns k + 1 (chunkMap the identity, chunkBase
// 0), and every block is a stream of its own (chunkStream [chunk] = chunk / ns), so that a pick has one ceiling per block.
struct VbrStage {
    const HostShape* hs = nullptr;
    int joint = 0, ns = 1;
    hipStream_t st = nullptr;
    const long long* chunkMap = nullptr;
    const int* chunkStream = nullptr;
};

int vbr_stage(mrc_handle* h, const std::string& who, int a, int b, int64_t n, int joint, void* stream, VbrStage* v) {
    if (n < 0 || n >= ((int64_t)1 << 28)) return fail(h, MRC_ERR_INVALID, who + ": n_frames negative or too large");
    MRC_TRY(get_shape(h, a, b, &v->hs));
    const DevShape& S = v->hs->dev;
    v->joint = joint ? 1 : 0;
    v->ns = joint ? 2 : 1;
    if (const char* why = chain_shape_misfit(S, v->ns)) return fail(h, MRC_ERR_INVALID, who + ": " + why);
    if (S.nBands > kMaxBands || vbr_lds_bytes(S, v->joint) > 60 * 1024)
        return fail(h, MRC_ERR_INVALID, who + ": block shape (a, b) outside what the VBR kernels hold in LDS");
    if (n == 0) return MRC_OK;
    MRC_HIP(h, hipSetDevice(h->device));
    v->st = pick_stream(h, stream);
    VbrBufs& V = h->vbr;
    const size_t chunks = (size_t)n * v->ns;
    StageLayout lay(16);
    const size_t oMap = lay.add<long long>(chunks), oStream = lay.add<int>(chunks), total = lay.total();
    MRC_HIP(h, V.stageMap.reserve(total));
    // page-locked staging, copied on the caller's stream: the previous call's copy must have read it before it is refilled
    MRC_HIP(h, V.stageCopied.create(hipEventDisableTiming));
    MRC_HIP(h, hipEventSynchronize(V.stageCopied));
    MRC_HIP(h, V.stagePin.reserve(total));
    char* host = (char*)V.stagePin.p;
    for (size_t c = 0; c < chunks; ++c) {
        reinterpret_cast<long long*>(host + oMap)[c] = (long long)c;
        reinterpret_cast<int*>(host + oStream)[c] = (int)(c / v->ns);
    }
    MRC_HIP(h, hipMemcpyAsync(V.stageMap.p, host, total, hipMemcpyHostToDevice, v->st));
    MRC_HIP(h, hipEventRecord(V.stageCopied, v->st));
    v->chunkMap = reinterpret_cast<const long long*>((char*)V.stageMap.p + oMap);
    v->chunkStream = reinterpret_cast<const int*>((char*)V.stageMap.p + oStream);
    return MRC_OK;
}

}  // namespace

extern "C" {

int mrc_encode_chained_target_nmr_pac(mrc_handle* h, int n_rates, const double* target_bits_per_sample,
                                      double target_nmr_total_db, int64_t n_streams, const int16_t* pcm_left,
                                      const int16_t* pcm_right, int64_t stream_stride, const int64_t* block_start,
                                      const int64_t* block_offset, const int32_t* block_a, const int32_t* block_b,
                                      int use_huffman, const uint32_t* num_samples, uint8_t* out, int64_t out_cap,
                                      int64_t* stream_byte_offset, int32_t* chosen, int32_t* met, double* nmr_total_db,
                                      double* nmr_max_db, int64_t* disturbed_blocks, int64_t* n_blocks, int64_t* total_bytes) {
    const TargetOut o{target_nmr_total_db, stream_byte_offset, chosen, met, nmr_total_db, nmr_max_db, disturbed_blocks, n_blocks};
    const ChainCall c{n_rates, target_bits_per_sample, n_streams, pcm_left, pcm_right, MRC_SAMPLES_PCM16, stream_stride, block_start,
                      block_offset, block_a, block_b, nullptr, use_huffman, 1, num_samples, nullptr, nullptr, nullptr, nullptr,
                      nullptr, nullptr};
    return target_call(h, __func__, c, o, out, out_cap, total_bytes, true);
}

int mrc_dev_encode_chained_target_nmr_pac(mrc_handle* h, int n_rates, const double* target_bits_per_sample,
                                          double target_nmr_total_db, int64_t n_streams, const int16_t* pcm_left,
                                          const int16_t* pcm_right, int64_t stream_stride, const int64_t* block_start,
                                          const int64_t* block_offset, const int32_t* block_a, const int32_t* block_b,
                                          int use_huffman, const uint32_t* num_samples, uint8_t* out, int64_t out_cap,
                                          int64_t* stream_byte_offset, int32_t* chosen, int32_t* met, double* nmr_total_db,
                                          double* nmr_max_db, int64_t* disturbed_blocks, int64_t* n_blocks, int64_t* total_bytes,
                                          void* stream) {
    const TargetOut o{target_nmr_total_db, stream_byte_offset, chosen, met, nmr_total_db, nmr_max_db, disturbed_blocks, n_blocks};
    const ChainCall c{n_rates, target_bits_per_sample, n_streams, pcm_left, pcm_right, MRC_SAMPLES_PCM16, stream_stride, block_start,
                      block_offset, block_a, block_b, nullptr, use_huffman, 1, num_samples, nullptr, nullptr, nullptr, nullptr,
                      nullptr, stream};
    return target_call(h, __func__, c, o, out, out_cap, total_bytes, false);
}

int mrc_get_target_ms(mrc_handle* h, double* ms) {
    if (!h || !ms) return MRC_ERR_INVALID;
    for (int i = 0; i < 4; ++i) ms[i] = h->target.ms[i];
    return MRC_OK;
}

int mrc_encode_vbr_nmr_pac(mrc_handle* h, double ceiling_db, int64_t n_streams, const int16_t* pcm_left, const int16_t* pcm_right,
                           int64_t stream_stride, const int64_t* block_start, const int64_t* block_offset,
                           const int32_t* block_a, const int32_t* block_b, int use_huffman, const uint32_t* num_samples,
                           uint8_t* out, int64_t out_cap, int64_t* stream_byte_offset, double* ceiling_ratio,
                           int64_t* capped_bands, int64_t* coded_bits, double* nmr_total_db, double* nmr_max_db,
                           int64_t* disturbed_blocks, int64_t* n_blocks, int64_t* total_bytes) {
    const VbrOut o{capped_bands, coded_bits, nmr_total_db, nmr_max_db, disturbed_blocks, n_blocks};
    const ChainCall c{1, nullptr, n_streams, pcm_left, pcm_right, MRC_SAMPLES_PCM16, stream_stride, block_start, block_offset,
                      block_a, block_b, nullptr, use_huffman, 1, num_samples, stream_byte_offset, nullptr, nullptr, nullptr,
                      total_bytes, nullptr};
    return vbr_call(h, __func__, ceiling_db, nullptr, c, o, out, out_cap, ceiling_ratio, true);
}

int mrc_dev_encode_vbr_nmr_pac(mrc_handle* h, double ceiling_db, int64_t n_streams, const int16_t* pcm_left,
                               const int16_t* pcm_right, int64_t stream_stride, const int64_t* block_start,
                               const int64_t* block_offset, const int32_t* block_a, const int32_t* block_b, int use_huffman,
                               const uint32_t* num_samples, uint8_t* out, int64_t out_cap, int64_t* stream_byte_offset,
                               double* ceiling_ratio, int64_t* capped_bands, int64_t* coded_bits, double* nmr_total_db,
                               double* nmr_max_db, int64_t* disturbed_blocks, int64_t* n_blocks, int64_t* total_bytes,
                               void* stream) {
    const VbrOut o{capped_bands, coded_bits, nmr_total_db, nmr_max_db, disturbed_blocks, n_blocks};
    const ChainCall c{1, nullptr, n_streams, pcm_left, pcm_right, MRC_SAMPLES_PCM16, stream_stride, block_start, block_offset,
                      block_a, block_b, nullptr, use_huffman, 1, num_samples, stream_byte_offset, nullptr, nullptr, nullptr,
                      total_bytes, stream};
    return vbr_call(h, __func__, ceiling_db, nullptr, c, o, out, out_cap, ceiling_ratio, false);
}

int mrc_encode_vbr_size_pac(mrc_handle* h, double ceiling_lo_db, double ceiling_step_db, int n_ceilings, const int64_t* target_bytes,
                            int64_t n_streams, const int16_t* pcm_left, const int16_t* pcm_right, int64_t stream_stride,
                            const int64_t* block_start, const int64_t* block_offset, const int32_t* block_a, const int32_t* block_b,
                            int use_huffman, const uint32_t* num_samples, uint8_t* out, int64_t out_cap, int64_t* stream_byte_offset,
                            int32_t* chosen, double* chosen_db, double* ceiling_ratio, int32_t* met, int32_t* probes,
                            int32_t* probe_index, int64_t* probe_bytes, int64_t* capped_bands, int64_t* coded_bits,
                            double* nmr_total_db, double* nmr_max_db, int64_t* disturbed_blocks, int64_t* n_blocks,
                            int64_t* total_bytes) {
    const VbrOut o{capped_bands, coded_bits, nmr_total_db, nmr_max_db, disturbed_blocks, n_blocks};
    const VbrSize Z{ceiling_lo_db, ceiling_step_db, n_ceilings, target_bytes, chosen, chosen_db, ceiling_ratio, met, probes,
                    probe_index, probe_bytes};
    const ChainCall c{1, nullptr, n_streams, pcm_left, pcm_right, MRC_SAMPLES_PCM16, stream_stride, block_start, block_offset,
                      block_a, block_b, nullptr, use_huffman, 1, num_samples, stream_byte_offset, nullptr, nullptr, nullptr,
                      total_bytes, nullptr};
    return vbr_call(h, __func__, 0.0, &Z, c, o, out, out_cap, ceiling_ratio, true);
}

int mrc_dev_encode_vbr_size_pac(mrc_handle* h, double ceiling_lo_db, double ceiling_step_db, int n_ceilings,
                                const int64_t* target_bytes, int64_t n_streams, const int16_t* pcm_left, const int16_t* pcm_right,
                                int64_t stream_stride, const int64_t* block_start, const int64_t* block_offset,
                                const int32_t* block_a, const int32_t* block_b, int use_huffman, const uint32_t* num_samples,
                                uint8_t* out, int64_t out_cap, int64_t* stream_byte_offset, int32_t* chosen, double* chosen_db,
                                double* ceiling_ratio, int32_t* met, int32_t* probes, int32_t* probe_index, int64_t* probe_bytes,
                                int64_t* capped_bands, int64_t* coded_bits, double* nmr_total_db, double* nmr_max_db,
                                int64_t* disturbed_blocks, int64_t* n_blocks, int64_t* total_bytes, void* stream) {
    const VbrOut o{capped_bands, coded_bits, nmr_total_db, nmr_max_db, disturbed_blocks, n_blocks};
    const VbrSize Z{ceiling_lo_db, ceiling_step_db, n_ceilings, target_bytes, chosen, chosen_db, ceiling_ratio, met, probes,
                    probe_index, probe_bytes};
    const ChainCall c{1, nullptr, n_streams, pcm_left, pcm_right, MRC_SAMPLES_PCM16, stream_stride, block_start, block_offset,
                      block_a, block_b, nullptr, use_huffman, 1, num_samples, stream_byte_offset, nullptr, nullptr, nullptr,
                      total_bytes, stream};
    return vbr_call(h, __func__, 0.0, &Z, c, o, out, out_cap, ceiling_ratio, false);
}

int mrc_get_vbr_size_ms(mrc_handle* h, double* ms) {
    if (!h || !ms) return MRC_ERR_INVALID;
    for (int i = 0; i < 5; ++i) ms[i] = h->vbr.sizeMs[i];
    return MRC_OK;
}

int mrc_get_vbr_ms(mrc_handle* h, double* ms) {
    if (!h || !ms) return MRC_ERR_INVALID;
    for (int i = 0; i < 4; ++i) ms[i] = h->vbr.ms[i];
    return MRC_OK;
}

int mrc_vbr_record_width(int joint) {
    DevShape one{};
    one.nBands = 1;
    return (int)(vbr_profile_bytes(one, joint ? 1 : 0) / sizeof(double));
}

int mrc_dev_vbr_alloc(mrc_handle* h, int a, int b, int64_t n_frames, int joint, double ceiling, const double* lines,
                      const int32_t* overall_scale, const int32_t* ms_switch, const double* source_lines,
                      const double* source_thresh, int32_t* bit_alloc, int32_t* scale_factor, uint16_t* mantissa16,
                      double* stat, int32_t* capped, void* stream) {
    if (!h) return MRC_ERR_INVALID;
    if (!lines || !overall_scale || (joint && !ms_switch) || !source_lines || !source_thresh)
        return fail(h, MRC_ERR_INVALID, "mrc_dev_vbr_alloc: null input (lines, overall_scale, ms_switch, source_lines or source_thresh)");
    if (!bit_alloc || !scale_factor || !mantissa16 || !stat || !capped)
        return fail(h, MRC_ERR_INVALID, "mrc_dev_vbr_alloc: null output (bit_alloc, scale_factor, mantissa16, stat or capped)");
    if (std::isnan(ceiling)) return fail(h, MRC_ERR_INVALID, "mrc_dev_vbr_alloc: ceiling is NaN");
    VbrStage v;
    MRC_TRY(vbr_stage(h, __func__, a, b, n_frames, joint, stream, &v));
    if (n_frames == 0) return MRC_OK;
    MRC_HIP(h, launch_vbr_alloc(v.hs->dev, v.joint, n_frames, 0, ceiling, lines, overall_scale, ms_switch, bit_alloc,
                                scale_factor, mantissa16, v.chunkMap, source_lines, source_thresh, stat, capped, 0, v.st));
    return MRC_OK;
}

int mrc_dev_vbr_profile(mrc_handle* h, int a, int b, int64_t n_frames, int joint, const double* lines,
                        const int32_t* overall_scale, const int32_t* ms_switch, const double* source_lines,
                        const double* source_thresh, double* ratios, uint32_t* picks, void* stream) {
    if (!h) return MRC_ERR_INVALID;
    if (!lines || !overall_scale || (joint && !ms_switch) || !source_lines || !source_thresh)
        return fail(h, MRC_ERR_INVALID, "mrc_dev_vbr_profile: null input (lines, overall_scale, ms_switch, source_lines or source_thresh)");
    if (!ratios || (joint && !picks)) return fail(h, MRC_ERR_INVALID, "mrc_dev_vbr_profile: null output (ratios or picks)");
    VbrStage v;
    MRC_TRY(vbr_stage(h, __func__, a, b, n_frames, joint, stream, &v));
    if (n_frames == 0) return MRC_OK;
    // states that the walk never reaches stay NaN (every byte 0xff)
    MRC_HIP(h, hipMemsetAsync(ratios, 0xff, (size_t)n_frames * vbr_profile_bytes(v.hs->dev, v.joint), v.st));
    MRC_HIP(h, launch_vbr_profile(v.hs->dev, v.joint, n_frames, 0, lines, overall_scale, ms_switch, source_lines, source_thresh,
                                  ratios, v.joint ? picks : nullptr, v.st));
    return MRC_OK;
}

int mrc_dev_vbr_pick(mrc_handle* h, int a, int b, int64_t n_frames, int joint, const double* ceilings, const double* lines,
                     const int32_t* overall_scale, const int32_t* ms_switch, const double* ratios, const uint32_t* picks,
                     int32_t* bit_alloc, int32_t* scale_factor, uint16_t* mantissa16, double* stat, int32_t* capped,
                     void* stream) {
    if (!h) return MRC_ERR_INVALID;
    if (!ceilings || !lines || !overall_scale || (joint && !ms_switch) || !ratios || (joint && !picks))
        return fail(h, MRC_ERR_INVALID, "mrc_dev_vbr_pick: null input (ceilings, lines, overall_scale, ms_switch, ratios or picks)");
    if (!bit_alloc || !scale_factor || !mantissa16 || !stat || !capped)
        return fail(h, MRC_ERR_INVALID, "mrc_dev_vbr_pick: null output (bit_alloc, scale_factor, mantissa16, stat or capped)");
    VbrStage v;
    MRC_TRY(vbr_stage(h, __func__, a, b, n_frames, joint, stream, &v));
    if (n_frames == 0) return MRC_OK;
    MRC_HIP(h, launch_vbr_pick(v.hs->dev, v.joint, n_frames, ceilings, v.chunkStream, lines, overall_scale, ms_switch, ratios,
                               v.joint ? picks : nullptr, bit_alloc, scale_factor, mantissa16, v.chunkMap, stat, capped, v.st));
    return MRC_OK;
}

}  // extern "C"
