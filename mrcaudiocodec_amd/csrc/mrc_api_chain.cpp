// C ABI, chained stream encode (include/mrc_hip.h: mrc_encode_chained_stream_pcm16_pac, mrc_dev_encode_chained_pac):
// the encode direction of the reference's command line (pacfileThem.py:1159-1214, Close() 973-984, file header 586-613)
// for whole stereo streams in ONE call, block shapes in, `.pac` bytes out -- and, with pcm_right == nullptr, the same loop
// for mono streams with WriteDataBlock in place of JointWriteDataBlock (pacfileThem.py:622-790, codecThem.py:205-231).
//
//   phase A   per block shape, ONE launch set over all blocks of all streams: windowed MDCT, overall scale, M/S switch,
//             SMRs, band peaks (the batch kernels) -- nothing here depends on the bit reservoir;
//   prep      per block: the bit allocation's grant events sorted (chain_prep_kernel);
//   phase B   one workgroup per stream walks its blocks in file order with the reservoir carried from block to block on
//             the device (chain_phase_b_kernel): bit allocation, scale factors, mantissas, Huffman pricing;
//   pack      per block shape plan / write kernels of the device packer around ONE prefix sum over all chunks in file
//             order, the file headers in front of every stream.
// No computation happens in this file.  An entry point puts its arguments into one ChainCall, checked once (check_call, the
// ladder's ladder_check in front of it); chained_slabs cuts the call into slabs, each the same ChainCall with the slab's fields
// overwritten; chained_core runs one slab: schedule_groups, phase A + prep queued, schedule_items while the device works,
// uploads, scan, pack, headers, chain_results.  The host-memory entry points are chained_host with one or several rates.
// The calls that measure their own output -- to a target noise-to-mask ratio, constant-quality VBR, VBR to a file size -- are
// in mrc_api_chain_measured.cpp.  They run through chained_slabs like every other call; what their slabs do beside encoding
// is one ChainMeasure (mrc_chain_call.hpp, ChainCall::measure), which chained_core asks three things: does the call allocate
// itself in place of the scan, what runs there or behind the pack, what is read from the events after the synchronise.
//
// Items, in file order per stream:  stereo  one joint block (two chunks) per block shape, Close()'s two one-channel blocks
//                                           (one chunk each);
//                                   mono    one one-channel block (one chunk) per block shape, Close()'s one block.
#include "mrc_chain_call.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace mrc;

namespace mrc {

const char* chain_shape_misfit(const DevShape& S, int nstream) {
    if (nstream * S.nBands > 64 || S.maxMantBits < 2 || S.maxMantBits > 16 || (S.halfN & 3))
        return "shape outside what the chained back end covers (<= 32 bands, 2..16 mantissa bits, lines a multiple of 4)";
    if (nstream * S.halfN > kChainMaxLinesPerItem)
        return "block too long for the chained back end (more than 2048 coded lines per block: n_mdct_lines <= 1024 in "
               "joint stereo)";
    return nullptr;
}

ChainGroupDev chain_group_desc(const HostShape& hs, int joint, const double* lines, const double* peak, const int* oscale,
                               const int* ms, const unsigned* ev, const unsigned* pre, int* bitAlloc, int* scaleFactor,
                               unsigned short* mant, int* table) {
    const DevShape& S = hs.dev;
    ChainGroupDev D{};
    D.joint = joint; D.nb = S.nBands; D.nstream = joint ? 2 : 1; D.nTot = D.nstream * S.nBands; D.M = S.halfN;
    D.K = S.maxMantBits - 1; D.nEv = (int)chain_events_per_block(S, joint); D.nScaleBits = S.nScaleBits;
    for (int v : hs.bandN) if (v > D.maxN) D.maxN = v;
    D.budgetMono = S.budgetMono; D.budgetJointPre = S.budgetJointPre; D.blkswA = S.blkswA; D.blkswB = S.blkswB;
    D.bandOfLine = S.bandOfLine; D.bandN = S.bandN;
    D.lines = lines; D.peak = peak; D.oscale = oscale; D.ms = ms; D.ev = ev; D.pre = pre;
    D.bitAlloc = bitAlloc; D.scaleFactor = scaleFactor; D.mant = mant; D.table = table;
    return D;
}

void chain_one_group(const ChainGroupDev& D, int64_t n, int64_t blocksPerStream, ChainGroupDev* desc, int32_t* items,
                     long long* itemStart) {
    *desc = D;
    for (int64_t i = 0; i < n; ++i) items[i] = (int32_t)i;                             // group 0, block i
    for (int64_t s = 0; s * blocksPerStream <= n; ++s) itemStart[s] = s * blocksPerStream;
}

}  // namespace mrc

namespace {

template <class T>
int upload(mrc_handle* h, DevBuf& buf, const std::vector<T>& v, hipStream_t st) {
    MRC_HIP(h, buf.reserve(v.empty() ? 1 : v.size() * sizeof(T)));
    if (!v.empty()) MRC_HIP(h, hipMemcpyAsync(buf.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st));
    return MRC_OK;
}

}  // namespace

extern "C" {

int mrc_get_chain_ms(mrc_handle* h, double* ms) {
    if (!h || !ms) return MRC_ERR_INVALID;
    for (int i = 0; i < 4; ++i) ms[i] = h->chainMs[i];
    return MRC_OK;
}

int64_t mrc_chain_out_bound_ex(mrc_handle* h, int n_channels, int64_t n_streams, const int64_t* block_start,
                               const int32_t* block_a, const int32_t* block_b, int with_flush, int with_headers) {
    if (!h || (n_channels != 1 && n_channels != 2) || n_streams < 0 || !block_start || !block_a || !block_b)
        return MRC_ERR_INVALID;
    const int L = h->cfg.n_mdct_lines, Sh = h->cfg.n_short;
    const int joint = n_channels == 2 ? 1 : 0;           // stereo: joint blocks; mono: one-channel blocks
    // a stream has four block shapes: their bounds once, not one band table per block
    const int sa[4] = {L, L, Sh, Sh}, sb[4] = {L, Sh, Sh, L};
    int64_t shapeBound[4];
    for (int g = 0; g < 4; ++g) shapeBound[g] = mrc_pack_bound(&h->cfg, sa[g], sb[g], n_channels, joint);
    int64_t total = 0;
    for (int64_t i = block_start[0]; i < block_start[n_streams]; ++i) {
        const int g = (block_a[i] == L ? 0 : 2) + ((block_a[i] == L) == (block_b[i] == L) ? 0 : 1);
        int64_t bnd = shapeBound[g];
        if (block_a[i] != sa[g] || block_b[i] != sb[g])
            bnd = mrc_pack_bound(&h->cfg, block_a[i], block_b[i], n_channels, joint);   // (refused later)
        if (bnd < 0) return MRC_ERR_INVALID;
        total += bnd;
    }
    if (with_flush) total += n_streams * mrc_pack_bound(&h->cfg, L, L, n_channels, 0);
    if (with_headers) total += n_streams * 128;
    return total;
}

int64_t mrc_chain_out_bound(mrc_handle* h, int64_t n_streams, const int64_t* block_start, const int32_t* block_a,
                            const int32_t* block_b, int with_flush, int with_headers) {
    return mrc_chain_out_bound_ex(h, 2, n_streams, block_start, block_a, block_b, with_flush, with_headers);
}

// The chained back end on the caller's lines and SMRs: what encode_host's few-block path launches behind encode_phase_a,
// with band_stats_kernel and ms_switch_kernel in place of the masking kernel's peaks and switch (as mrc_dev_alloc_quant).
int mrc_dev_alloc_quant_chained(mrc_handle* h, int a, int b, int64_t n_frames, int joint, int64_t blocks_per_stream,
                                int use_huffman, const double* lines, const int32_t* overall_scale, const double* smr,
                                const int32_t* reservoir_in, int32_t* ms_switch, int32_t* bit_alloc, int32_t* scale_factor,
                                uint16_t* mantissa16, int32_t* huff_table, int32_t* reservoir_out, int32_t* reservoir_trace,
                                void* stream) {
    if (!h || !lines || !overall_scale || !smr || !bit_alloc || !scale_factor || !mantissa16 || !reservoir_out ||
        (joint && !ms_switch) || n_frames < 0)
        return fail(h, MRC_ERR_INVALID, "mrc_dev_alloc_quant_chained: null argument or negative frame count");
    if (blocks_per_stream < 1 || n_frames % blocks_per_stream)
        return fail(h, MRC_ERR_INVALID, "mrc_dev_alloc_quant_chained: n_frames must be a multiple of blocks_per_stream >= 1");
    if (n_frames >= ((int64_t)1 << 28)) return fail(h, MRC_ERR_INVALID, "mrc_dev_alloc_quant_chained: too many blocks");
    if ((reinterpret_cast<uintptr_t>(lines) & 15) || (reinterpret_cast<uintptr_t>(mantissa16) & 7))
        return fail(h, MRC_ERR_INVALID, "mrc_dev_alloc_quant_chained: lines must be 16-byte aligned, mantissa16 8-byte aligned");
    const HostShape* hs;
    MRC_TRY(get_shape(h, a, b, &hs));
    const DevShape& S = hs->dev;
    joint = joint ? 1 : 0;
    const int nstream = joint ? 2 : 1;
    if (const char* why = chain_shape_misfit(S, nstream))
        return fail(h, MRC_ERR_INVALID, std::string("mrc_dev_alloc_quant_chained: ") + why);
    const int64_t n = n_frames, nStreams = n / blocks_per_stream;
    if (n == 0) return MRC_OK;
    MRC_HIP(h, hipSetDevice(h->device));
    hipStream_t st = pick_stream(h, stream);
    SmallBatchBufs& B = h->smallBatch;
    const size_t nEv = chain_events_per_block(S, joint);
    StageLayout lay(16);
    const size_t oDesc = lay.add<ChainGroupDev>(1), oItems = lay.add<int32_t>((size_t)n),
                 oStart = lay.add<long long>((size_t)nStreams + 1), total = lay.total();
    MRC_HIP(h, B.ctl.reserve(total));
    MRC_HIP(h, B.ev.reserve((size_t)n * nEv * sizeof(unsigned)));
    MRC_HIP(h, B.pre.reserve((size_t)n * (nEv + 1) * sizeof(unsigned)));
    if (!huff_table) MRC_HIP(h, B.table.reserve((size_t)n * nstream * sizeof(int32_t)));
    MRC_HIP(h, h->ws.peak.reserve(alloc_workspace_bytes(S, n, joint)));
    double* peak = h->ws.peak.as<double>();
    char* dev = (char*)B.ctl.p;
    // page-locked staging, copied on the caller's stream: the previous call's copy must have read it before it is refilled
    MRC_HIP(h, B.ctlCopied.create(hipEventDisableTiming));
    MRC_HIP(h, hipEventSynchronize(B.ctlCopied));
    MRC_HIP(h, B.ctlPin.reserve(total));
    char* host = (char*)B.ctlPin.p;
    chain_one_group(chain_group_desc(*hs, joint, lines, peak, overall_scale, ms_switch, B.ev.as<unsigned>(),
                                     B.pre.as<unsigned>(), bit_alloc, scale_factor, mantissa16,
                                     huff_table ? huff_table : B.table.as<int32_t>()),
                    n, blocks_per_stream, reinterpret_cast<ChainGroupDev*>(host + oDesc),
                    reinterpret_cast<int32_t*>(host + oItems), reinterpret_cast<long long*>(host + oStart));
    MRC_HIP(h, hipMemcpyAsync(dev, host, total, hipMemcpyHostToDevice, st));
    MRC_HIP(h, hipEventRecord(B.ctlCopied, st));
    if (!reservoir_in) MRC_HIP(h, hipMemsetAsync(reservoir_out, 0, (size_t)nStreams * sizeof(int32_t), st));
    else if (reservoir_in != reservoir_out)
        MRC_HIP(h, hipMemcpyAsync(reservoir_out, reservoir_in, (size_t)nStreams * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    MRC_HIP(h, launch_band_peaks(S, n, joint, lines, peak, st));
    if (joint)                                                      // on the UNSCALED L / R lines (codecThem.py:436)
        MRC_HIP(h, launch_ms_switch(n, S.nBands, S.msLeaves, S.msInternal, S.msPlan, lines, lines + S.halfN,
                                    4 * (int64_t)S.halfN, S.halfN, ms_switch, st));
    MRC_HIP(h, launch_chain_prep(S, joint, n, smr, joint ? ms_switch : nullptr, B.ev.as<unsigned>(), B.pre.as<unsigned>(),
                                 h->chainForceFallback ? 1 : 0, st));
    MRC_HIP(h, launch_chain_phase_b(nStreams, 1, (const ChainGroupDev*)(dev + oDesc), (const int*)(dev + oItems),
                                    (const long long*)(dev + oStart), reservoir_out, reservoir_trace, n,
                                    use_huffman ? 1 : 0, h->chainThreads, st));
    return MRC_OK;
}

}  // extern "C"

namespace {

// Step 1: the shapes' tables, the schedule's own refusals, the blocks sorted into their shape groups -- all phase A needs
// (that every stream has a block is chained_slabs' check: its slab plan counts on it first)
int schedule_groups(mrc_handle* h, const ChainCall& c, ChainSchedule* q) {
    const int L = h->cfg.n_mdct_lines, Sh = h->cfg.n_short, nch = c.nch();
    const int shapeA[kChainGroups] = {L, L, Sh, Sh, L}, shapeB[kChainGroups] = {L, Sh, Sh, L, L};
    q->nGroups = c.with_flush ? kChainGroups : kChainGroups - 1;
    for (int g = 0; g < q->nGroups; ++g) {
        MRC_TRY(get_shape(h, shapeA[g], shapeB[g], &q->hs[g]));
        if (const char* why = chain_shape_misfit(q->hs[g]->dev, (g == 4 || nch == 1) ? 1 : 2))
            return fail(h, MRC_ERR_INVALID, std::string("mrc_encode_chained: ") + why);
    }
    const int64_t b0 = c.block_start[0], nB = c.n_blocks();
    q->groupOf.resize((size_t)nB);
    q->tailOff.resize((size_t)c.n_streams);
    q->offs[0].reserve((size_t)nB);
    for (int64_t s = 0; s < c.n_streams; ++s) {
        const int64_t i1 = c.block_start[s + 1];
        for (int64_t i = c.block_start[s]; i < i1; ++i) {
            const int a = c.block_a[i], b = c.block_b[i];
            int g = -1;
            for (int k = 0; k < 4; ++k) if (a == shapeA[k] && b == shapeB[k]) { g = k; break; }   // (L == Sh: group 0)
            if (g < 0) return fail(h, MRC_ERR_INVALID, "mrc_encode_chained: block shape is not one of (L,L), (L,S), (S,S), (S,L)");
            const int64_t off = c.block_offset[i];
            if (off < 0 || off + a + b > c.stream_stride)
                return fail(h, MRC_ERR_INVALID, "mrc_encode_chained: block reaches outside its stream");
            if (q->offs[g].size() >= (size_t)1 << 28) return fail(h, MRC_ERR_INVALID, "mrc_encode_chained: too many blocks of one shape");
            q->groupOf[(size_t)(i - b0)] = (uint8_t)g;
            q->offs[g].push_back(s * c.stream_stride + off);
        }
        if (c.with_flush) {
            if (c.block_b[i1 - 1] != L)
                return fail(h, MRC_ERR_INVALID, "mrc_encode_chained: a stream must end with a long block (the reference's "
                                                "Close() assumes it, pacfileThem.py:973-984)");
            q->tailOff[(size_t)s] = c.block_offset[i1 - 1] + c.block_a[i1 - 1];
        }
    }
    return MRC_OK;
}

// Step 2: what only the serial scan and the packer need.  chained_core calls it once phase A is queued, so that the device
// works while the host builds it.
int schedule_items(mrc_handle* h, const ChainCall& c, ChainSchedule* q) {
    const int R = c.n_rates, nch = c.nch();
    const int64_t nS = c.n_streams, b0 = c.block_start[0], nItems = c.n_items(), nChunks = c.n_chunks();
    q->items.resize((size_t)nItems);
    q->itemStart.resize((size_t)nS + 1); q->firstChunk.resize((size_t)nS);
    q->itemChunk.resize((size_t)nItems + 1);
    q->chunkStream.resize((size_t)(R * nChunks));
    q->resIn.assign((size_t)(R * nS), 0);
    for (int g = 0; g < 4; ++g) q->chunkMap[g].resize(R * nch * q->offs[g].size());
    if (c.with_flush) q->chunkMap[4].resize((size_t)(R * nch * nS));
    int64_t it = 0, ch = 0;
    size_t idx[kChainGroups] = {};
    for (int64_t s = 0; s < nS; ++s) {
        q->itemStart[(size_t)s] = it;
        q->firstChunk[(size_t)s] = ch;
        for (int64_t i = c.block_start[s]; i < c.block_start[s + 1]; ++i) {
            const int g = q->groupOf[(size_t)(i - b0)];
            const size_t k = idx[g]++;
            q->items[(size_t)it] = (int32_t)((unsigned)g << 28 | (unsigned)k);
            q->itemChunk[(size_t)it] = ch;
            for (int chn = 0; chn < nch; ++chn) {
                q->chunkMap[g][nch * k + chn] = ch;
                q->chunkStream[(size_t)ch++] = (int32_t)s;
            }
            ++it;
        }
        if (c.with_flush)
            for (int chn = 0; chn < nch; ++chn) {                 // codec.Encode: channel after channel
                q->items[(size_t)it] = (int32_t)(4u << 28 | (unsigned)(nch * s + chn));
                q->chunkMap[4][(size_t)(nch * s + chn)] = ch;
                q->itemChunk[(size_t)it] = ch;
                q->chunkStream[(size_t)ch] = (int32_t)s;
                ++ch; ++it;
            }
    }
    q->itemStart[(size_t)nS] = it;
    q->itemChunk[(size_t)nItems] = ch;
    if (c.reservoir_in) q->resIn.assign(c.reservoir_in, c.reservoir_in + R * nS);
    // rates after the first: their chunks behind all of the previous rate's, (rate, stream) the "stream" of each
    for (int r = 1; r < R; ++r) {
        for (int64_t k = 0; k < nChunks; ++k) q->chunkStream[(size_t)(r * nChunks + k)] = (int32_t)(r * nS) + q->chunkStream[(size_t)k];
        for (int g = 0; g < q->nGroups; ++g) {
            const size_t n1 = q->chunkMap[g].size() / R;            // (the group's chunks of one rate)
            for (size_t k = 0; k < n1; ++k) q->chunkMap[g][r * n1 + k] = r * nChunks + q->chunkMap[g][k];
        }
        for (int64_t s = 0; s < nS; ++s) q->firstChunk.push_back(r * nChunks + q->firstChunk[(size_t)s]);
    }
    if (c.num_samples) {
        // file headers (pacfileThem.py:586-613): one built by mrc_pac_header; the streams differ only in the sample count
        // (bytes 10..13, little endian, with the reference's padding rule, pacfileThem.py:595-597: padded when it ALREADY is
        // a multiple of nMDCTLines); the same headers in front of every rate's streams
        uint8_t one[256];
        int64_t len = 0;
        if (mrc_pac_header(&h->cfg, nch, c.num_samples[0], one, sizeof(one), &len) != MRC_OK || len < 14)
            return fail(h, MRC_ERR_INVALID, "mrc_encode_chained: mrc_pac_header failed");
        q->hdrLen = (int)len;
        q->hdr.resize((size_t)(R * nS) * len);
        for (int64_t s = 0; s < R * nS; ++s) {
            uint8_t* dst = q->hdr.data() + s * len;
            std::memcpy(dst, one, (size_t)len);
            uint32_t ns = c.num_samples[s % nS];
            if (ns % (uint32_t)h->cfg.n_mdct_lines == 0) ns += (uint32_t)h->cfg.n_mdct_lines;
            for (int k = 0; k < 4; ++k) dst[10 + k] = (uint8_t)(ns >> (8 * k));
        }
    }
    if (c.item_byte_offset) q->pos.resize((size_t)(R * nChunks) + 1);
    q->streamPos.resize((size_t)(R * nS));
    q->resOut.resize((size_t)(R * nS));
    return MRC_OK;
}

// What was read back, as the caller's outputs: rate r's bytes reach from its first stream's start to the next rate's (to the
// end when it is the last); rate_base[r] is where they start in the slab's buffer, every offset is relative to it.
void chain_results(const ChainCall& c, const ChainSchedule& q, int64_t* rate_base) {
    const int64_t nS = c.n_streams, nItems = c.n_items(), nChunks = c.n_chunks();
    for (int r = 0; r < c.n_rates; ++r) {
        const long long base = q.streamPos[(size_t)(r * nS)];
        const long long end = r + 1 < c.n_rates ? q.streamPos[(size_t)((r + 1) * nS)] : q.total;
        c.total_bytes[r] = end - base;
        rate_base[r] = base;
        int64_t* so = c.stream_byte_offset + r * (nS + 1);
        for (int64_t s = 0; s < nS; ++s) so[s] = q.streamPos[(size_t)(r * nS + s)] - base;
        so[nS] = end - base;
        if (c.item_byte_offset) {
            int64_t* io = c.item_byte_offset + r * (nItems + 1);
            for (int64_t i = 0; i < nItems; ++i) io[i] = q.pos[(size_t)(r * nChunks + q.itemChunk[(size_t)i])] - base;
            io[nItems] = end - base;
        }
    }
    if (c.reservoir_out) std::memcpy(c.reservoir_out, q.resOut.data(), q.resOut.size() * sizeof(int32_t));
}

// One SLAB of a chained encode: all of the call's streams, every buffer sized for exactly these blocks (chained_slabs cuts a
// call into slabs and checked that every stream has a block).  The bytes of all rates go to out [out_cap], device memory.
int chained_core(mrc_handle* h, const ChainCall& c, uint8_t* out, int64_t out_cap, int64_t* rate_base) {
    const mrc_config& cfg = h->cfg;
    const int R = c.n_rates, L = cfg.n_mdct_lines, nch = c.nch();
    const int64_t nS = c.n_streams, nItems = c.n_items(), nChunks = c.n_chunks();
    // (a call that allocates itself needs no SMRs, band peaks and event lists: phase A stops at the M/S switch)
    const bool scans = !(c.measure && c.measure->allocates());
    ChainSchedule q;
    std::vector<ChainGroupDev> desc((size_t)R * kChainGroups);   // [rate][group]
    MRC_TRY(schedule_groups(h, c, &q));
    MRC_HIP(h, hipSetDevice(h->device));
    hipStream_t st = pick_stream(h, c.stream);
    ChainBufs& C = h->chain;
    MRC_HIP(h, C.evT.create());
    DrainGuard guard{{st}};                              // (declared behind q and desc: they outlive every queued copy)
    MRC_HIP(h, hipEventRecord(C.evT[0], st));
    if (c.with_flush) {
        // the tail offsets ride in the offsets buffer of group 4 (its blocks are laid out explicitly, stride 2 L)
        MRC_TRY(upload(h, C.g[4].offsets, q.tailOff, st));
        MRC_HIP(h, C.flushPcm.reserve((size_t)nS * nch * 2 * L * c.sample_bytes()));
        MRC_HIP(h, launch_chain_flush_gather(nS, L, c.pcm_left, c.pcm_right, c.sample_format, c.stream_stride,
                                             C.g[4].offsets.as<long long>(), C.flushPcm.p, st));
    }
    // ---- phase A + prep, per block shape
    int64_t count[kChainGroups] = {};
    for (int g = 0; g < q.nGroups; ++g) {
        const DevShape& S = q.hs[g]->dev;
        // stereo: groups 0-3 joint (two chunks per block), Close() two one-channel items; mono: every item one channel
        const int joint = (g == 4 || nch == 1) ? 0 : 1, nsig = joint ? 4 : 1, nstream = joint ? 2 : 1;
        const int64_t m = g == 4 ? nch * nS : (int64_t)q.offs[g].size();
        count[g] = m;
        ChainGroupBufs& B = C.g[g];
        const int nTot = nstream * S.nBands, nEv = (int)chain_events_per_block(S, joint);
        if (m > 0) {
            if (g != 4) MRC_TRY(upload(h, B.offsets, q.offs[g], st));
            MRC_HIP(h, B.lines.reserve((size_t)m * nsig * S.halfN * sizeof(double)));
            MRC_HIP(h, B.oscale.reserve((size_t)m * nsig * sizeof(int32_t)));
            if (joint) MRC_HIP(h, B.ms.reserve((size_t)m * S.nBands * sizeof(int32_t)));
            if (scans) {
                MRC_HIP(h, B.smr.reserve((size_t)m * nsig * S.nBands * sizeof(double)));
                MRC_HIP(h, B.peak.reserve((size_t)m * nsig * S.nBands * sizeof(double)));
                MRC_HIP(h, B.ev.reserve((size_t)m * nEv * sizeof(unsigned)));
                MRC_HIP(h, B.pre.reserve((size_t)m * (nEv + 1) * sizeof(unsigned)));
            }
            MRC_HIP(h, B.bitAlloc.reserve((size_t)R * m * nTot * sizeof(int32_t)));          // (phase B's planes: one per rate)
            MRC_HIP(h, B.scaleFactor.reserve((size_t)R * m * nTot * sizeof(int32_t)));
            MRC_HIP(h, B.mant.reserve((size_t)R * m * nstream * S.halfN * sizeof(uint16_t)));
            MRC_HIP(h, B.table.reserve((size_t)R * m * nstream * sizeof(int32_t)));
            double* smr = scans ? B.smr.as<double>() : nullptr;
            if (g == 4)
                MRC_TRY(encode_phase_a(h, S, m, C.flushPcm.p, nullptr, c.sample_format, 2 * (int64_t)L, nullptr, B.lines.as<double>(),
                                       B.oscale.as<int32_t>(), nullptr, smr, B.peak.as<double>(), st, false));
            else                                             // (pcm_right == nullptr: the mono kernels, no M/S switch)
                MRC_TRY(encode_phase_a(h, S, m, c.pcm_left, c.pcm_right, c.sample_format, 0, B.offsets.as<int64_t>(),
                                       B.lines.as<double>(), B.oscale.as<int32_t>(), joint ? B.ms.as<int32_t>() : nullptr,
                                       smr, B.peak.as<double>(), st, false));
            if (scans)
                MRC_HIP(h, launch_chain_prep(S, joint, m, B.smr.as<double>(), joint ? B.ms.as<int32_t>() : nullptr,
                                         B.ev.as<unsigned>(), B.pre.as<unsigned>(),
                                         h->chainForceFallback ? 1 : 0, st));
        }
        for (int r = 0; r < R; ++r) {
            // rate r: the shared phase-A data, its own budgets and output planes
            ChainGroupDev& D = desc[(size_t)r * kChainGroups + g];
            D = chain_group_desc(*q.hs[g], joint, B.lines.as<double>(), B.peak.as<double>(), B.oscale.as<int32_t>(),
                                 joint ? B.ms.as<int32_t>() : nullptr, B.ev.as<unsigned>(), B.pre.as<unsigned>(),
                                 B.bitAlloc.as<int32_t>() + r * m * nTot, B.scaleFactor.as<int32_t>() + r * m * nTot,
                                 B.mant.as<unsigned short>() + r * m * nstream * S.halfN, B.table.as<int32_t>() + r * m * nstream);
            if (c.rates) shape_budgets(cfg, c.rates[r], S.a, S.b, S.nBands, &D.budgetMono, &D.budgetJointPre);
        }
    }
    // ---- the rest of the schedule, built while the device is busy with phase A, and its uploads
    MRC_TRY(schedule_items(h, c, &q));
    MRC_TRY(upload(h, C.items, q.items, st));
    MRC_TRY(upload(h, C.itemStart, q.itemStart, st));
    MRC_TRY(upload(h, C.reservoir, q.resIn, st));
    MRC_TRY(upload(h, C.chunkStream, q.chunkStream, st));
    MRC_TRY(upload(h, C.hdr, q.hdr, st));
    MRC_TRY(upload(h, C.firstChunk, q.firstChunk, st));
    for (int g = 0; g < q.nGroups; ++g)
        if (count[g] > 0) MRC_TRY(upload(h, C.g[g].chunkMap, q.chunkMap[g], st));
    if (c.reservoir_trace) MRC_HIP(h, C.resTrace.reserve((size_t)(R * nItems) * sizeof(int32_t)));
    MRC_TRY(upload(h, C.groupDesc, desc, st));
    MRC_HIP(h, hipEventRecord(C.evT[1], st));
    // ---- phase B: the serial scan per stream and rate, or the call's own allocation (no reservoir: nothing is carried)
    if (!scans) MRC_TRY(c.measure->in_place_of_scan(h, c, q, count, st));
    else
        MRC_HIP(h, launch_chain_phase_b(nS, R, C.groupDesc.as<ChainGroupDev>(), C.items.as<int>(), C.itemStart.as<long long>(),
                                        C.reservoir.as<int>(), c.reservoir_trace ? C.resTrace.as<int>() : nullptr, nItems,
                                        c.use_huffman ? 1 : 0, h->chainThreads, st));
    MRC_HIP(h, hipEventRecord(C.evT[2], st));
    if (h->sensOn)                                       // MRC_OPT_SENSITIVITY: the scan's decisions, group by group
        for (int g = 0; g < q.nGroups; ++g) {
            ChainGroupBufs& B = C.g[g];
            const int joint = desc[g].joint;                 // (one rate: the ladder refuses the option)
            MRC_HIP(h, launch_sensitivity(q.hs[g]->dev, count[g], joint, B.lines.as<double>(), B.oscale.as<int32_t>(),
                                          B.smr.as<double>(), B.peak.as<double>(), joint ? B.ms.as<int32_t>() : nullptr,
                                          B.bitAlloc.as<int32_t>(), B.scaleFactor.as<int32_t>(),
                                          h->sens.as<unsigned long long>(), nullptr, st));
        }
    // ---- pack: plan per (rate, shape), ONE prefix sum over the chunks of all rates in file order, write per (rate, shape)
    const PackTables& tables = host_pack_tables();
    const int64_t nChunksAll = R * nChunks;
    MRC_HIP(h, C.packWs.reserve(pack_workspace_bytes(nChunksAll)));
    const PackWs W = pack_ws_views(C.packWs.p, nChunksAll);
    MRC_HIP(h, hipMemsetAsync(W.errorFlag, 0, sizeof(int), st));
    PackParams P[kChainGroups];
    for (int g = 0; g < q.nGroups; ++g) {
        const int joint = desc[g].joint;
        P[g] = pack_params(cfg, q.hs[g]->dev.a, q.hs[g]->dev.b, joint ? 2 : 1, joint, c.use_huffman);
        if (!count[g]) continue;
        for (int r = 0; r < R; ++r) {                           // (a mono item is a one-channel block)
            const ChainGroupDev& D = desc[(size_t)r * kChainGroups + g];
            // (the scan chose the tables; without it calculateHuffmanGain's choice is the packer's, as for independent frames)
            MRC_HIP(h, launch_pack_plan(q.hs[g]->dev, P[g], tables, count[g], D.bitAlloc, D.mant, MRC_MANTISSA_I16,
                                        scans ? D.table : nullptr, D.table,
                                        nullptr, W, C.g[g].chunkMap.as<long long>() + r * (q.chunkMap[g].size() / R),
                                        all_bands_non_empty(*q.hs[g]), st));
        }
    }
    MRC_HIP(h, launch_pack_scan(nChunksAll, 0, W, nullptr, c.num_samples ? C.chunkStream.as<int>() : nullptr, q.hdrLen, st));
    for (int g = 0; g < q.nGroups; ++g) {
        if (!count[g]) continue;
        ChainGroupBufs& B = C.g[g];
        const int bound = (int)(mrc_pack_bound(&cfg, q.hs[g]->dev.a, q.hs[g]->dev.b, 1, P[g].joint) - 4);
        for (int r = 0; r < R; ++r) {
            const ChainGroupDev& D = desc[(size_t)r * kChainGroups + g];
            MRC_HIP(h, launch_pack_write(q.hs[g]->dev, P[g], tables, count[g], B.oscale.as<int>(), P[g].joint ? B.ms.as<int>() : nullptr,
                                         D.scaleFactor, D.bitAlloc, D.mant, MRC_MANTISSA_I16, D.table, W,
                                         B.chunkMap.as<long long>() + r * (q.chunkMap[g].size() / R), out, (long long)out_cap, bound,
                                         all_bands_non_empty(*q.hs[g]), st));
        }
    }
    // ---- the file headers (num_samples given), and the start of every (rate, stream)'s bytes
    MRC_HIP(h, C.streamPos.reserve((size_t)(R * nS) * sizeof(long long)));
    MRC_HIP(h, launch_chain_headers(R * nS, q.hdrLen, C.hdr.as<unsigned char>(), C.firstChunk.as<long long>(), W.pos, out,
                                    (long long)out_cap, C.streamPos.as<long long>(), st));
    MRC_HIP(h, hipEventRecord(C.evT[3], st));
    if (c.measure) MRC_TRY(c.measure->behind_pack(h, c, q, count, st));
    // ---- read back: stream starts (the position of every chunk only if the caller asked for them), total, error flag,
    // reservoirs
    if (c.item_byte_offset)
        MRC_HIP(h, hipMemcpyAsync(q.pos.data(), W.pos, q.pos.size() * sizeof(long long), hipMemcpyDeviceToHost, st));
    MRC_HIP(h, hipMemcpyAsync(q.streamPos.data(), C.streamPos.p, q.streamPos.size() * sizeof(long long), hipMemcpyDeviceToHost, st));
    MRC_HIP(h, hipMemcpyAsync(&q.total, W.total, sizeof(q.total), hipMemcpyDeviceToHost, st));
    MRC_HIP(h, hipMemcpyAsync(&q.bad, W.errorFlag, sizeof(q.bad), hipMemcpyDeviceToHost, st));
    MRC_HIP(h, hipMemcpyAsync(q.resOut.data(), C.reservoir.p, q.resOut.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (c.reservoir_trace)
        MRC_HIP(h, hipMemcpyAsync(c.reservoir_trace, C.resTrace.p, (size_t)(R * nItems) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    MRC_HIP(h, hipStreamSynchronize(st));
    for (int i = 0; i < 4; ++i)                          // phase A + prep | scan | pack | all three
        MRC_HIP(h, C.evT.elapsed(i < 3 ? i : 0, i < 3 ? i + 1 : 3, &h->chainMs[i]));
    if (c.measure) MRC_TRY(c.measure->read_events(h));
    chain_results(c, q, rate_base);
    if (q.bad & 3) return fail(h, MRC_ERR_INVALID, "mrc_encode_chained: internal error (table id / chunk size out of range)");
    if (q.total > out_cap || (q.bad & 4)) return fail(h, MRC_ERR_NOMEM, "mrc_encode_chained: out_cap too small (see total_bytes)");
    return MRC_OK;
}

}  // namespace

namespace mrc {

// ---- slabs (round 4).  Phase A keeps ~45 KB of device memory per joint long block (the MDCT lines of four signals, SMRs,
// events, outputs) and the worst-case output bound is 13 KB per block: a call over a 2^18-hop file would hold 18 GB.  A call is
// therefore cut into SLABS of at most h->chainSlabBlocks blocks, each a chained_core of its own whose buffers are reused by
// the next: whole streams while they fit (their files stay contiguous in the output), a stream longer than a slab alone in
// consecutive TIME slabs -- the reservoir goes from slab to slab as it goes from block to block (codecThem.py:274,503), the
// header travels with the first slab, Close()'s blocks with the last.  `sink` receives each slab's bytes.
static std::vector<Slab> plan_slabs(int64_t n_streams, const int64_t* block_start, int64_t cap) {
    std::vector<Slab> v;
    int64_t s = 0;
    while (s < n_streams) {
        const int64_t nb = block_start[s + 1] - block_start[s];
        if (nb > cap) {                                  // one long stream: time slabs
            for (int64_t i = block_start[s]; i < block_start[s + 1]; i += cap) {
                const int64_t e = std::min<int64_t>(i + cap, block_start[s + 1]);
                v.push_back({s, 1, i, e, i == block_start[s], e == block_start[s + 1], true});
            }
            ++s;
            continue;
        }
        int64_t e = s, blocks = 0;
        while (e < n_streams && block_start[e + 1] - block_start[e] <= cap && blocks + (block_start[e + 1] - block_start[e]) <= cap) {
            blocks += block_start[e + 1] - block_start[e];
            ++e;
        }
        v.push_back({s, e - s, block_start[s], block_start[e], true, true, false});
        s = e;
    }
    return v;
}

// How many blocks a slab of a rate ladder takes: phase A's buffers are shared by the rates, the scan's planes, the packer's
// workspace and the output bound are per rate -- so that a ladder's slab holds about the device memory of a one-rate slab
// of `cap` blocks (per block of the long shape), whatever the number of rates.
static int64_t ladder_slab_blocks(mrc_handle* h, int64_t cap, int n_rates, int nch) {
    if (n_rates <= 1) return cap;
    const int L = h->cfg.n_mdct_lines;
    const HostShape* hs = nullptr;
    if (get_shape(h, L, L, &hs) != MRC_OK) return cap;                  // (the call itself says why)
    const DevShape& S = hs->dev;
    const int joint = nch == 2 ? 1 : 0, nsig = joint ? 4 : 1, nTot = nch * S.nBands;
    const int64_t nEv = (int64_t)chain_events_per_block(S, joint);
    const int64_t shared = (int64_t)nsig * S.halfN * 8 + (int64_t)nsig * S.nBands * 16 + nsig * 4 + S.nBands * 4 + (2 * nEv + 1) * 4 + 12;
    const int64_t perRate = 2 * (int64_t)nTot * 4 + (int64_t)nch * S.halfN * 2 + nch * 4 +
                            nch * (12 + (int64_t)(pack_workspace_bytes((int64_t)1 << 20) >> 20)) + mrc_pack_bound(&h->cfg, L, L, nch, joint);
    return std::max<int64_t>(1, cap * (shared + perRate) / (shared + n_rates * perRate));
}

// mrc_encode_vbr_size_pac keeps vbr_profile_kernel's record of every block of a slab beside phase A's data: its slab takes
// as many blocks fewer as hold the device memory of a one-rate slab of `cap` blocks (per block of the long shape).
int64_t vbr_size_slab_blocks(mrc_handle* h, int nch) {
    const int64_t cap = h->chainSlabBlocks;
    if (cap <= 0) return (int64_t)1 << 40;
    const int L = h->cfg.n_mdct_lines;
    const HostShape* hs = nullptr;
    if (get_shape(h, L, L, &hs) != MRC_OK) return cap;                  // (the call itself says why)
    const DevShape& S = hs->dev;
    const int joint = nch == 2 ? 1 : 0, nsig = joint ? 4 : 1, nTot = nch * S.nBands;
    const int64_t block = (int64_t)nsig * S.halfN * 8 + nsig * 4 + S.nBands * 4 + 2 * (int64_t)nTot * 4 + (int64_t)nch * S.halfN * 2 +
                          nch * 4 + nch * 16 + mrc_pack_bound(&h->cfg, L, L, nch, joint);
    const int64_t record = (int64_t)vbr_profile_bytes(S, joint) + (joint ? S.nBands * 4 : 0);
    return std::max<int64_t>(1, cap * block / (block + record));
}

static int64_t slab_cap(mrc_handle* h, int n_rates, int nch) {
    return h->chainSlabBlocks > 0 ? ladder_slab_blocks(h, h->chainSlabBlocks, n_rates, nch) : (int64_t)1 << 40;
}

// A chained encode cut into slabs (mrc_chain_call.hpp says what sink and after receive)
int chained_slabs(mrc_handle* h, const ChainCall& c, const int64_t* out_cap, uint8_t* direct_out, const ChainSink& sink,
                  const ChainAfter& after) {
    const int R = c.n_rates, nch = c.nch();
    const int64_t nS = c.n_streams;
    for (int r = 0; r < R; ++r) { c.total_bytes[r] = 0; c.stream_byte_offset[r * (nS + 1)] = 0; }
    if (nS == 0) return MRC_OK;
    for (int64_t s = 0; s < nS; ++s)                     // (the slab plan and every size below count on it)
        if (c.block_start[s + 1] <= c.block_start[s]) return fail(h, MRC_ERR_INVALID, "mrc_encode_chained: every stream needs at least one block");
    const int64_t nItemsAll = c.n_items();
    const std::vector<Slab> slabs = plan_slabs(nS, c.block_start, c.slabBlocks > 0 ? c.slabBlocks : slab_cap(h, R, nch));
    ChainBufs& C = h->chain;
    int64_t itemBase = 0;
    std::vector<int64_t> written((size_t)R, 0), slabTotal((size_t)R), base((size_t)R);
    std::vector<char> overflow((size_t)R, 0);
    double ms[4] = {0, 0, 0, 0};
    std::vector<int64_t> sOff, iOff;
    std::vector<int32_t> resInSlab, resOutSlab, trace;
    for (const Slab& sl : slabs) {
        // the slab's call: the caller's, with its streams, its blocks, and outputs of its own that are stitched below
        ChainCall sc = c;
        const size_t skip = (size_t)sl.s0 * c.stream_stride * c.sample_bytes();
        const int64_t timeStart[2] = {sl.i0, sl.i1};
        sc.slab = &sl;
        sc.n_streams = sl.ns;
        sc.pcm_left = (const char*)c.pcm_left + skip;
        if (c.pcm_right) sc.pcm_right = (const char*)c.pcm_right + skip;
        sc.block_start = sl.timeSlab ? timeStart : c.block_start + sl.s0;
        sc.with_flush = c.with_flush && sl.last;
        sc.num_samples = (c.num_samples && sl.first) ? c.num_samples + sl.s0 : nullptr;
        // its reservoirs in: what the stream's previous time slab left ([R][1]), or the caller's rows of these streams
        if (sl.timeSlab && !sl.first) resInSlab = resOutSlab;
        else if (c.reservoir_in) {
            resInSlab.resize((size_t)(R * sl.ns));
            for (int r = 0; r < R; ++r)
                for (int64_t s = 0; s < sl.ns; ++s) resInSlab[(size_t)(r * sl.ns + s)] = c.reservoir_in[r * nS + sl.s0 + s];
        }
        if (c.reservoir_in || (sl.timeSlab && !sl.first)) sc.reservoir_in = resInSlab.data();
        const int64_t nItems = sc.n_items();
        sOff.assign((size_t)(R * (sl.ns + 1)), 0);
        if (c.item_byte_offset) iOff.assign((size_t)(R * (nItems + 1)), 0);
        resOutSlab.assign((size_t)(R * sl.ns), 0);
        if (c.reservoir_trace) trace.assign((size_t)(R * nItems), 0);
        sc.stream_byte_offset = sOff.data();
        sc.item_byte_offset = c.item_byte_offset ? iOff.data() : nullptr;
        sc.reservoir_out = resOutSlab.data();
        sc.reservoir_trace = c.reservoir_trace ? trace.data() : nullptr;
        sc.total_bytes = slabTotal.data();
        uint8_t* dst;
        int64_t slabCap;
        if (direct_out && !overflow[0]) { dst = direct_out + written[0]; slabCap = out_cap[0] - written[0]; }
        else {
            const int64_t bound = mrc_chain_out_bound_ex(h, nch, sl.ns, sc.block_start, c.block_a, c.block_b, sc.with_flush,
                                                         sc.num_samples != nullptr);
            if (bound < 0) return fail(h, MRC_ERR_INVALID, "mrc_encode_chained: block shape out of range");
            MRC_HIP(h, hipSetDevice(h->device));
            MRC_HIP(h, C.out.reserve((size_t)(R * bound) + 1));
            dst = C.out.as<uint8_t>(); slabCap = R * bound;
        }
        int rc = chained_core(h, sc, dst, slabCap, base.data());
        if (rc == MRC_ERR_NOMEM && direct_out) overflow[0] = 1;          // the caller's buffer is full: sizes only from here on
        else if (rc != MRC_OK) return rc;
        for (int i = 0; i < 4; ++i) ms[i] += h->chainMs[i];
        for (int r = 0; r < R; ++r) {
            int64_t* so = c.stream_byte_offset + r * (nS + 1);
            const int64_t* slabSo = sOff.data() + r * (sl.ns + 1);
            // (a time slab behind its stream's first leaves the stream's start alone and moves its end and reservoir on)
            for (int64_t s = sl.first ? 0 : 1; s <= sl.ns; ++s) so[sl.s0 + s] = written[(size_t)r] + slabSo[s];
            if (c.reservoir_out)
                for (int64_t s = 0; s < sl.ns; ++s) c.reservoir_out[r * nS + sl.s0 + s] = resOutSlab[(size_t)(r * sl.ns + s)];
            if (c.item_byte_offset)
                for (int64_t i = 0; i <= nItems; ++i)
                    c.item_byte_offset[r * (nItemsAll + 1) + itemBase + i] = written[(size_t)r] + iOff[(size_t)(r * (nItems + 1) + i)];
            if (c.reservoir_trace && nItems)
                std::memcpy(c.reservoir_trace + r * nItemsAll + itemBase, trace.data() + r * nItems, (size_t)nItems * sizeof(int32_t));
            if (!direct_out && !overflow[(size_t)r]) {
                if (written[(size_t)r] + slabTotal[(size_t)r] > out_cap[r]) overflow[(size_t)r] = 1;
                else if (sink) MRC_TRY(sink(sl, r, dst + base[(size_t)r], slabTotal[(size_t)r], written[(size_t)r]));
            }
            written[(size_t)r] += slabTotal[(size_t)r];
        }
        if (after) MRC_TRY(after(sl, sOff.data(), base.data(), dst));
        itemBase += nItems;
    }
    for (int i = 0; i < 4; ++i) h->chainMs[i] = ms[i];
    bool full = false;
    for (int r = 0; r < R; ++r) {
        c.total_bytes[r] = written[(size_t)r];
        c.stream_byte_offset[r * (nS + 1) + nS] = written[(size_t)r];
        full = full || overflow[(size_t)r] || written[(size_t)r] > out_cap[r];
    }
    if (R == 1 && slabs.size() == 1 && !direct_out) C.lastTotal = written[0];   // (one slab: its bytes are all in C.out, mrc_chain_fetch_output)
    if (full) return fail(h, MRC_ERR_NOMEM, "mrc_encode_chained: out_cap too small (see total_bytes)");
    return MRC_OK;
}

void forget_held_output(mrc_handle* h) {
    h->chain.lastTotal = -1;
    h->chain.lastSrc = nullptr;
}

int check_call(mrc_handle* h, const char* who, const ChainCall& c, uint8_t* const* out, const int64_t* out_cap) {
    bool ok = h && c.n_streams >= 0 && c.pcm_left && c.stream_stride > 0 && c.block_start && c.block_offset &&
              c.block_a && c.block_b && out && out_cap && c.stream_byte_offset && c.total_bytes &&
              (c.sample_format == MRC_SAMPLES_F64 || c.sample_format == MRC_SAMPLES_PCM16);
    for (int r = 0; ok && r < c.n_rates; ++r) ok = out[r] && out_cap[r] >= 0;
    if (!ok) return fail(h, MRC_ERR_INVALID, std::string(who) + ": bad argument");
    forget_held_output(h);
    return MRC_OK;
}

int rate_count_check(mrc_handle* h, const std::string& w, int n_rates) {
    if (n_rates < 1 || n_rates > MRC_MAX_RATES) return fail(h, MRC_ERR_INVALID, w + ": n_rates must lie in 1..MRC_MAX_RATES (16)");
    return MRC_OK;
}

int rate_check(mrc_handle* h, const std::string& w, const double* rates, int r, bool ascending) {
    if (!std::isfinite(rates[r]) || !(rates[r] > 0.0) || rates[r] > 64.0)
        return fail(h, MRC_ERR_INVALID, w + ": target_bits_per_sample[" + std::to_string(r) + "] must be finite and in (0, 64]");
    if (ascending && r && !(rates[r] > rates[r - 1]))
        return fail(h, MRC_ERR_INVALID, w + ": target_bits_per_sample must be strictly ascending (entry " + std::to_string(r) + " is not)");
    return MRC_OK;
}

// the ladder's own refusals, in front of check_call
static int ladder_check(mrc_handle* h, const char* who, int n_rates, const double* rates, uint8_t* const* out, const int64_t* out_cap,
                 int64_t* total_bytes) {
    const std::string w(who);
    if (!h) return MRC_ERR_INVALID;
    MRC_TRY(rate_count_check(h, w, n_rates));
    if (!rates || !out || !out_cap || !total_bytes)
        return fail(h, MRC_ERR_INVALID, w + ": target_bits_per_sample, out, out_cap and total_bytes must not be NULL");
    for (int r = 0; r < n_rates; ++r) {
        MRC_TRY(rate_check(h, w, rates, r, false));
        if (!out[r]) return fail(h, MRC_ERR_INVALID, w + ": out[" + std::to_string(r) + "] is NULL");
        if (out_cap[r] < 0) return fail(h, MRC_ERR_INVALID, w + ": out_cap[" + std::to_string(r) + "] is negative");
    }
    if (h->sensOn)
        return fail(h, MRC_ERR_INVALID, w + ": MRC_OPT_SENSITIVITY is on (the certificate covers one rate: encode each rate on its own)");
    return MRC_OK;
}

int stage_pcm(mrc_handle* h, const ChainCall& c) {
    ChainBufs& C = h->chain;
    const size_t pcmBytes = (size_t)c.n_streams * c.stream_stride * c.sample_bytes();
    MRC_HIP(h, C.pcmL.reserve(pcmBytes ? pcmBytes : 1));
    if (c.pcm_right) MRC_HIP(h, C.pcmR.reserve(pcmBytes ? pcmBytes : 1));    // (mono streams: no right channel)
    DrainGuard guard{{h->stream}};
    if (pcmBytes) {
        MRC_HIP(h, hipMemcpyAsync(C.pcmL.p, c.pcm_left, pcmBytes, hipMemcpyHostToDevice, h->stream));
        if (c.pcm_right) MRC_HIP(h, hipMemcpyAsync(C.pcmR.p, c.pcm_right, pcmBytes, hipMemcpyHostToDevice, h->stream));
    }
    return MRC_OK;
}

// The host-memory entry points (the one-rate one: a ladder of one rate with rates == nullptr): the PCM staged in the handle's
// device buffers, every slab packed into the handle's output buffer (sized for the slab's worst case), rate r's bytes copied
// behind the previous slab's in out[r], which only has to hold what the streams really pack to.
int chained_host(mrc_handle* h, const char* who, ChainCall c, uint8_t* const* out, const int64_t* out_cap, const ChainAfter& after) {
    MRC_TRY(check_call(h, who, c, out, out_cap));
    MRC_HIP(h, hipSetDevice(h->device));
    MRC_TRY(stage_pcm(h, c));
    ChainBufs& C = h->chain;
    hipStream_t st = h->stream;                          // (c.stream is null: the launches are queued on it too)
    c.pcm_left = C.pcmL.p;
    if (c.pcm_right) c.pcm_right = C.pcmR.p;
    int rc = chained_slabs(h, c, out_cap, nullptr, [out, st, h](const Slab&, int r, uint8_t* buf, int64_t n, int64_t at) {
        if (n) MRC_HIP(h, hipMemcpyAsync(out[r] + at, buf, (size_t)n, hipMemcpyDeviceToHost, st));
        MRC_HIP(h, hipStreamSynchronize(st));            // (the next slab reuses the buffer)
        return (int)MRC_OK;
    }, after);
    if (rc == MRC_ERR_NOMEM)
        return fail(h, MRC_ERR_NOMEM, std::string(who) + (c.rates ? ": an out_cap too small (see total_bytes)"
                                                                  : ": out_cap too small (see total_bytes; mrc_chain_fetch_output)"));
    return rc;
}

}  // namespace mrc

extern "C" {

int mrc_dev_encode_chained_pac(mrc_handle* h, int64_t n_streams, const void* pcm_left, const void* pcm_right,
                               int sample_format, int64_t stream_stride, const int64_t* block_start, const int64_t* block_offset,
                               const int32_t* block_a, const int32_t* block_b, const int32_t* reservoir_in,
                               int use_huffman, int with_flush, const uint32_t* num_samples, uint8_t* out, int64_t out_cap,
                               int64_t* stream_byte_offset, int64_t* item_byte_offset, int32_t* reservoir_out,
                               int32_t* reservoir_trace, int64_t* total_bytes, void* stream) {
    const ChainCall c{1, nullptr, n_streams, pcm_left, pcm_right, sample_format, stream_stride, block_start, block_offset,
                      block_a, block_b, reservoir_in, use_huffman, with_flush, num_samples, stream_byte_offset, item_byte_offset,
                      reservoir_out, reservoir_trace, total_bytes, stream};
    MRC_TRY(check_call(h, __func__, c, &out, &out_cap));
    return chained_slabs(h, c, &out_cap, out, {}, {});
}

int mrc_encode_chained_stream_pac(mrc_handle* h, int64_t n_streams, const void* pcm_left, const void* pcm_right,
                                  int sample_format, int64_t stream_stride, const int64_t* block_start,
                                  const int64_t* block_offset, const int32_t* block_a, const int32_t* block_b,
                                  const int32_t* reservoir_in, int use_huffman, int with_flush, const uint32_t* num_samples,
                                  uint8_t* out, int64_t out_cap, int64_t* stream_byte_offset, int64_t* item_byte_offset,
                                  int32_t* reservoir_out, int32_t* reservoir_trace, int64_t* total_bytes) {
    const ChainCall c{1, nullptr, n_streams, pcm_left, pcm_right, sample_format, stream_stride, block_start, block_offset,
                      block_a, block_b, reservoir_in, use_huffman, with_flush, num_samples, stream_byte_offset, item_byte_offset,
                      reservoir_out, reservoir_trace, total_bytes, nullptr};
    return chained_host(h, __func__, c, &out, &out_cap);
}

int mrc_encode_chained_ladder_pac(mrc_handle* h, int n_rates, const double* target_bits_per_sample, int64_t n_streams,
                                  const void* pcm_left, const void* pcm_right, int sample_format, int64_t stream_stride,
                                  const int64_t* block_start, const int64_t* block_offset, const int32_t* block_a,
                                  const int32_t* block_b, const int32_t* reservoir_in, int use_huffman, int with_flush,
                                  const uint32_t* num_samples, uint8_t* const* out, const int64_t* out_cap,
                                  int64_t* stream_byte_offset, int64_t* item_byte_offset, int32_t* reservoir_out,
                                  int32_t* reservoir_trace, int64_t* total_bytes) {
    MRC_TRY(ladder_check(h, __func__, n_rates, target_bits_per_sample, out, out_cap, total_bytes));
    const ChainCall c{n_rates, target_bits_per_sample, n_streams, pcm_left, pcm_right, sample_format, stream_stride, block_start,
                      block_offset, block_a, block_b, reservoir_in, use_huffman, with_flush, num_samples, stream_byte_offset,
                      item_byte_offset, reservoir_out, reservoir_trace, total_bytes, nullptr};
    return chained_host(h, __func__, c, out, out_cap);
}

int mrc_dev_encode_chained_ladder_pac(mrc_handle* h, int n_rates, const double* target_bits_per_sample, int64_t n_streams,
                                      const void* pcm_left, const void* pcm_right, int sample_format, int64_t stream_stride,
                                      const int64_t* block_start, const int64_t* block_offset, const int32_t* block_a,
                                      const int32_t* block_b, const int32_t* reservoir_in, int use_huffman, int with_flush,
                                      const uint32_t* num_samples, uint8_t* const* out, const int64_t* out_cap,
                                      int64_t* stream_byte_offset, int64_t* item_byte_offset, int32_t* reservoir_out,
                                      int32_t* reservoir_trace, int64_t* total_bytes, void* stream) {
    MRC_TRY(ladder_check(h, __func__, n_rates, target_bits_per_sample, out, out_cap, total_bytes));
    const ChainCall c{n_rates, target_bits_per_sample, n_streams, pcm_left, pcm_right, sample_format, stream_stride, block_start,
                      block_offset, block_a, block_b, reservoir_in, use_huffman, with_flush, num_samples, stream_byte_offset,
                      item_byte_offset, reservoir_out, reservoir_trace, total_bytes, stream};
    MRC_TRY(check_call(h, __func__, c, out, out_cap));
    hipStream_t st = pick_stream(h, stream);
    // rate r's bytes of a slab go behind the previous slab's in out[r], ordered on `st` before the next slab packs
    int rc = chained_slabs(h, c, out_cap, nullptr, [out, st, h](const Slab&, int r, uint8_t* buf, int64_t n, int64_t at) {
        if (n) MRC_HIP(h, hipMemcpyAsync(out[r] + at, buf, (size_t)n, hipMemcpyDeviceToDevice, st));
        return (int)MRC_OK;
    }, {});
    if (rc == MRC_OK || rc == MRC_ERR_NOMEM) MRC_HIP(h, hipStreamSynchronize(st));
    if (rc == MRC_ERR_NOMEM) return fail(h, MRC_ERR_NOMEM, std::string(__func__) + ": an out_cap too small (see total_bytes)");
    return rc;
}

int mrc_chain_fetch_output(mrc_handle* h, uint8_t* out, int64_t out_cap, int64_t* total_bytes) {
    if (!h || !out || !total_bytes) return fail(h, MRC_ERR_INVALID, "mrc_chain_fetch_output: bad argument");
    ChainBufs& C = h->chain;
    if (C.lastTotal < 0) return fail(h, MRC_ERR_INVALID, "mrc_chain_fetch_output: no output of a chained call is held");
    *total_bytes = C.lastTotal;
    if (C.lastTotal > out_cap) return fail(h, MRC_ERR_NOMEM, "mrc_chain_fetch_output: out_cap too small (see total_bytes)");
    MRC_HIP(h, hipSetDevice(h->device));
    if (C.lastTotal)
        MRC_HIP(h, hipMemcpyAsync(out, C.lastSrc ? C.lastSrc : C.out.p, (size_t)C.lastTotal, hipMemcpyDeviceToHost, h->stream));
    MRC_HIP(h, hipStreamSynchronize(h->stream));
    return MRC_OK;
}

int mrc_encode_chained_stream_pcm16_pac(mrc_handle* h, int64_t n_streams, const int16_t* pcm_left, const int16_t* pcm_right,
                                        int64_t stream_stride, const int64_t* block_start, const int64_t* block_offset,
                                        const int32_t* block_a, const int32_t* block_b, const int32_t* reservoir_in,
                                        int use_huffman, int with_flush, const uint32_t* num_samples, uint8_t* out,
                                        int64_t out_cap, int64_t* stream_byte_offset, int64_t* item_byte_offset,
                                        int32_t* reservoir_out, int32_t* reservoir_trace, int64_t* total_bytes) {
    return mrc_encode_chained_stream_pac(h, n_streams, pcm_left, pcm_right, MRC_SAMPLES_PCM16, stream_stride, block_start,
                                         block_offset, block_a, block_b, reservoir_in, use_huffman, with_flush, num_samples,
                                         out, out_cap, stream_byte_offset, item_byte_offset, reservoir_out, reservoir_trace,
                                         total_bytes);
}

}  // extern "C"
