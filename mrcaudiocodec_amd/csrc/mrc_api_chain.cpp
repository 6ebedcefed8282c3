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
// mrc_encode_chained_target_nmr_pac (end of the file) is a ladder whose slabs also measure their rungs (ChainCall::nmr) and
// whose caller receives the chosen rung alone.  mrc_encode_vbr_nmr_pac (behind it) is a one-rate call whose slabs allocate
// per band against a noise-to-mask ceiling (ChainCall::vbr, vbr_slab) in place of the event lists and the serial scan;
// mrc_encode_vbr_size_pac is that call with the ceiling searched per stream (ChainVbr::size: the slab records every band's walk
// once and bisects a grid of ceilings over the record, vbr_size_search).
//
// Items, in file order per stream:  stereo  one joint block (two chunks) per block shape, Close()'s two one-channel blocks
//                                           (one chunk each);
//                                   mono    one one-channel block (one chunk) per block shape, Close()'s one block.
#include "mrc_handle.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
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

}  // extern "C"

namespace {

// One chained encode as its entry point received it, in the order of include/mrc_hip.h.  n_rates bit rates (rates == nullptr:
// one, the handle's target_bits_per_sample): phase A and the event lists once, the scan and the packer per (rate, stream).
// pcm_right == nullptr: mono streams.  Every per-stream / per-item array holds n_rates rows: reservoir_in / reservoir_out
// [R][n_streams], stream_byte_offset [R][n_streams + 1], item_byte_offset [R][n_items + 1], reservoir_trace [R][n_items],
// total_bytes [R]; byte offsets are relative to the start of their rate's output.  Where the bytes go is the layers' own.
struct ChainNmr;
struct ChainVbr;
struct ChainCall {
    int n_rates; const double* rates;
    int64_t n_streams;
    const void *pcm_left, *pcm_right; int sample_format; int64_t stream_stride;
    const int64_t *block_start, *block_offset; const int32_t *block_a, *block_b;
    const int32_t* reservoir_in; int use_huffman, with_flush; const uint32_t* num_samples;
    int64_t *stream_byte_offset, *item_byte_offset; int32_t *reservoir_out, *reservoir_trace; int64_t* total_bytes;
    void* stream;
    ChainNmr* nmr = nullptr;         // mrc_encode_chained_target_nmr_pac: every slab also measures its rungs (target_nmr_slab)
    ChainVbr* vbr = nullptr;         // mrc_encode_vbr_nmr_pac: no budget, no scan -- every slab allocates per band (vbr_slab)
    int64_t slabBlocks = 0;          // the slab capacity of this call where it is not slab_cap's (mrc_encode_vbr_size_pac)
    int nch() const { return pcm_right ? 2 : 1; }
    size_t sample_bytes() const { return sample_format == MRC_SAMPLES_PCM16 ? sizeof(int16_t) : sizeof(double); }
    int64_t n_blocks() const { return block_start[n_streams] - block_start[0]; }
    int64_t n_items() const { return n_blocks() + (with_flush ? nch() * n_streams : 0); }   // Close(): a block per channel
    int64_t n_chunks() const { return n_items() + (nch() - 1) * n_blocks(); }               // a joint block: two chunks
};

// The host side of one chained_core.  Queued copies read and write these vectors: a ChainSchedule is declared in front of
// the DrainGuard of the stream they are queued on.
struct ChainSchedule {
    // the block shapes of the reference's block switching (pacfileThem.py:1192-1210); group 4: Close()'s blocks
    int nGroups = 0;
    const HostShape* hs[kChainGroups] = {};
    // schedule_groups, before phase A: the group of every block, the sample offsets of every group's blocks, Close()'s
    std::vector<uint8_t> groupOf;
    std::vector<int64_t> offs[kChainGroups];
    std::vector<long long> tailOff;
    // schedule_items, while phase A runs: items (group << 28 | index inside the group) per stream in file order, the chunk
    // of every item, the (rate, stream) of every chunk, the chunks of every group, the file headers
    std::vector<int32_t> items, chunkStream, resIn;
    std::vector<long long> itemStart, firstChunk, itemChunk, chunkMap[kChainGroups];
    std::vector<uint8_t> hdr;
    int hdrLen = 0;
    // read back: chunk positions (only if the caller asked for item offsets), (rate, stream) starts, reservoirs
    std::vector<long long> pos, streamPos;
    std::vector<int32_t> resOut;
    long long total = 0;
    int bad = 0;
};

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

// mrc_encode_chained_target_nmr_pac (below): the NMR of the slab's rungs from the planes the scan just wrote, and its device time
int target_nmr_slab(mrc_handle* h, const ChainCall& c, const ChainSchedule& q, const int64_t* count, hipStream_t st);
int target_nmr_time(mrc_handle* h, const ChainCall& c);
// mrc_encode_vbr_nmr_pac (below): the slab's allocation in place of the scan -- source analysis, vbr_alloc_kernel -- and its time
int vbr_slab(mrc_handle* h, const ChainCall& c, const ChainSchedule& q, const int64_t* count, hipStream_t st);
int vbr_time(mrc_handle* h, const ChainCall& c);

// One SLAB of a chained encode: all of the call's streams, every buffer sized for exactly these blocks (chained_slabs cuts a
// call into slabs and checked that every stream has a block).  The bytes of all rates go to out [out_cap], device memory.
int chained_core(mrc_handle* h, const ChainCall& c, uint8_t* out, int64_t out_cap, int64_t* rate_base) {
    const mrc_config& cfg = h->cfg;
    const int R = c.n_rates, L = cfg.n_mdct_lines, nch = c.nch();
    const int64_t nS = c.n_streams, nItems = c.n_items(), nChunks = c.n_chunks();
    ChainSchedule q;
    std::vector<ChainGroupDev> desc((size_t)R * kChainGroups);   // [rate][group]
    MRC_TRY(schedule_groups(h, c, &q));
    MRC_HIP(h, hipSetDevice(h->device));
    hipStream_t st = pick_stream(h, c.stream);
    ChainBufs& C = h->chain;
    for (auto& e : C.evT) if (!e) MRC_HIP(h, hipEventCreate(&e));
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
            if (!c.vbr) {                                    // (the VBR call needs no SMRs: it allocates against measured noise)
                MRC_HIP(h, B.smr.reserve((size_t)m * nsig * S.nBands * sizeof(double)));
                MRC_HIP(h, B.peak.reserve((size_t)m * nsig * S.nBands * sizeof(double)));
                MRC_HIP(h, B.ev.reserve((size_t)m * nEv * sizeof(unsigned)));
                MRC_HIP(h, B.pre.reserve((size_t)m * (nEv + 1) * sizeof(unsigned)));
            }
            MRC_HIP(h, B.bitAlloc.reserve((size_t)R * m * nTot * sizeof(int32_t)));          // (phase B's planes: one per rate)
            MRC_HIP(h, B.scaleFactor.reserve((size_t)R * m * nTot * sizeof(int32_t)));
            MRC_HIP(h, B.mant.reserve((size_t)R * m * nstream * S.halfN * sizeof(uint16_t)));
            MRC_HIP(h, B.table.reserve((size_t)R * m * nstream * sizeof(int32_t)));
            if (c.vbr) {                                     // phase A without its last step: lines, overall scales, M/S switch
                if (g == 4)
                    MRC_HIP(h, launch_mdct(S, m, C.flushPcm.p, nullptr, c.sample_format, 2 * (int64_t)L, nullptr, true,
                                           B.lines.as<double>(), B.oscale.as<int32_t>(), st));
                else
                    MRC_HIP(h, launch_mdct(S, m, c.pcm_left, c.pcm_right, c.sample_format, 0, B.offsets.as<int64_t>(), true,
                                           B.lines.as<double>(), B.oscale.as<int32_t>(), st));
                if (joint)
                    MRC_HIP(h, launch_ms_switch(m, S.nBands, S.msLeaves, S.msInternal, S.msPlan, B.lines.as<double>(),
                                                B.lines.as<double>() + S.halfN, 4 * (int64_t)S.halfN, S.halfN, B.ms.as<int32_t>(), st));
            } else if (g == 4)
                MRC_TRY(encode_phase_a(h, S, m, C.flushPcm.p, nullptr, c.sample_format, 2 * (int64_t)L, nullptr, B.lines.as<double>(),
                                       B.oscale.as<int32_t>(), nullptr, B.smr.as<double>(), B.peak.as<double>(), st, false));
            else                                             // (pcm_right == nullptr: the mono kernels, no M/S switch)
                MRC_TRY(encode_phase_a(h, S, m, c.pcm_left, c.pcm_right, c.sample_format, 0, B.offsets.as<int64_t>(),
                                       B.lines.as<double>(), B.oscale.as<int32_t>(), joint ? B.ms.as<int32_t>() : nullptr,
                                       B.smr.as<double>(), B.peak.as<double>(), st, false));
            if (!c.vbr)
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
    // ---- phase B: the serial scan per stream and rate
    if (c.vbr) MRC_TRY(vbr_slab(h, c, q, count, st));    // (no reservoir: nothing is carried from block to block)
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
            // (the scan chose the tables; the VBR call leaves calculateHuffmanGain's choice to the packer, as independent frames do)
            MRC_HIP(h, launch_pack_plan(q.hs[g]->dev, P[g], tables, count[g], D.bitAlloc, D.mant, MRC_MANTISSA_I16,
                                        c.vbr ? nullptr : D.table, D.table,
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
    if (c.nmr) MRC_TRY(target_nmr_slab(h, c, q, count, st));
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
    for (int i = 0; i < 4; ++i) {                        // phase A + prep | scan | pack | all three
        float ms = 0.f;
        MRC_HIP(h, hipEventElapsedTime(&ms, C.evT[i < 3 ? i : 0], C.evT[i < 3 ? i + 1 : 3]));
        h->chainMs[i] = ms;
    }
    if (c.nmr) MRC_TRY(target_nmr_time(h, c));
    if (c.vbr) MRC_TRY(vbr_time(h, c));
    chain_results(c, q, rate_base);
    if (q.bad & 3) return fail(h, MRC_ERR_INVALID, "mrc_encode_chained: internal error (table id / chunk size out of range)");
    if (q.total > out_cap || (q.bad & 4)) return fail(h, MRC_ERR_NOMEM, "mrc_encode_chained: out_cap too small (see total_bytes)");
    return MRC_OK;
}

// ---- slabs (round 4).  Phase A keeps ~45 KB of device memory per joint long block (the MDCT lines of four signals, SMRs,
// events, outputs) and the worst-case output bound is 13 KB per block: a call over a 2^18-hop file would hold 18 GB.  A call is
// therefore cut into SLABS of at most h->chainSlabBlocks blocks, each a chained_core of its own whose buffers are reused by
// the next: whole streams while they fit (their files stay contiguous in the output), a stream longer than a slab alone in
// consecutive TIME slabs -- the reservoir goes from slab to slab as it goes from block to block (codecThem.py:274,503), the
// header travels with the first slab, Close()'s blocks with the last.  `sink` receives each slab's bytes.
struct Slab { int64_t s0, ns; int64_t i0, i1; bool first, last, timeSlab; };

std::vector<Slab> plan_slabs(int64_t n_streams, const int64_t* block_start, int64_t cap) {
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
int64_t ladder_slab_blocks(mrc_handle* h, int64_t cap, int n_rates, int nch) {
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

int64_t slab_cap(mrc_handle* h, int n_rates, int nch) {
    return h->chainSlabBlocks > 0 ? ladder_slab_blocks(h, h->chainSlabBlocks, n_rates, nch) : (int64_t)1 << 40;
}

struct NoAfter { int operator()(const Slab&, const int64_t*, const int64_t*, const uint8_t*) const { return MRC_OK; } };

// A chained encode cut into slabs.  out_cap[r] is the room of rate r's output.  direct_out (one rate): a device buffer of
// out_cap[0] bytes the slabs write into in place; null: every slab packs into the handle's buffer and
// sink(rate r, its slab bytes are at `buf` on the device, n of them, they belong at byte `at` of rate r's output) -> status;
// after(the slab, its stream_byte_offset [R][ns + 1], where each rate's bytes start in `buf`, buf) -> status, once per slab
// behind its sinks
template <class Sink, class After>
int chained_slabs(mrc_handle* h, const ChainCall& c, const int64_t* out_cap, uint8_t* direct_out, Sink sink, After after) {
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
                else MRC_TRY(sink(r, dst + base[(size_t)r], slabTotal[(size_t)r], written[(size_t)r]));
            }
            written[(size_t)r] += slabTotal[(size_t)r];
        }
        MRC_TRY(after(sl, sOff.data(), base.data(), dst));
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

// The one argument check of a chained call: all that can be refused without reading the schedule (out, out_cap: an entry
// per rate).  A call that passes serves no earlier call's output any more (mrc_chain_fetch_output), whatever becomes of it.
int check_call(mrc_handle* h, const char* who, const ChainCall& c, uint8_t* const* out, const int64_t* out_cap) {
    bool ok = h && c.n_streams >= 0 && c.pcm_left && c.stream_stride > 0 && c.block_start && c.block_offset &&
              c.block_a && c.block_b && out && out_cap && c.stream_byte_offset && c.total_bytes &&
              (c.sample_format == MRC_SAMPLES_F64 || c.sample_format == MRC_SAMPLES_PCM16);
    for (int r = 0; ok && r < c.n_rates; ++r) ok = out[r] && out_cap[r] >= 0;
    if (!ok) return fail(h, MRC_ERR_INVALID, std::string(who) + ": bad argument");
    h->chain.lastTotal = -1;
    h->chain.lastSrc = nullptr;
    return MRC_OK;
}

// the ladder's own refusals, in front of check_call
int ladder_check(mrc_handle* h, const char* who, int n_rates, const double* rates, uint8_t* const* out, const int64_t* out_cap,
                 int64_t* total_bytes) {
    const std::string w(who);
    if (!h) return MRC_ERR_INVALID;
    if (n_rates < 1 || n_rates > MRC_MAX_RATES) return fail(h, MRC_ERR_INVALID, w + ": n_rates must lie in 1..MRC_MAX_RATES (16)");
    if (!rates || !out || !out_cap || !total_bytes)
        return fail(h, MRC_ERR_INVALID, w + ": target_bits_per_sample, out, out_cap and total_bytes must not be NULL");
    for (int r = 0; r < n_rates; ++r) {
        if (!std::isfinite(rates[r]) || !(rates[r] > 0.0) || rates[r] > 64.0)
            return fail(h, MRC_ERR_INVALID, w + ": target_bits_per_sample[" + std::to_string(r) + "] must be finite and in (0, 64]");
        if (!out[r]) return fail(h, MRC_ERR_INVALID, w + ": out[" + std::to_string(r) + "] is NULL");
        if (out_cap[r] < 0) return fail(h, MRC_ERR_INVALID, w + ": out_cap[" + std::to_string(r) + "] is negative");
    }
    if (h->sensOn)
        return fail(h, MRC_ERR_INVALID, w + ": MRC_OPT_SENSITIVITY is on (the certificate covers one rate: encode each rate on its own)");
    return MRC_OK;
}

// stage the host PCM of a host-memory entry point in the handle's device buffers
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
template <class After = NoAfter>
int chained_host(mrc_handle* h, const char* who, ChainCall c, uint8_t* const* out, const int64_t* out_cap, After after = After{}) {
    MRC_TRY(check_call(h, who, c, out, out_cap));
    MRC_HIP(h, hipSetDevice(h->device));
    MRC_TRY(stage_pcm(h, c));
    ChainBufs& C = h->chain;
    hipStream_t st = h->stream;                          // (c.stream is null: the launches are queued on it too)
    c.pcm_left = C.pcmL.p;
    if (c.pcm_right) c.pcm_right = C.pcmR.p;
    int rc = chained_slabs(h, c, out_cap, nullptr, [out, st, h](int r, uint8_t* buf, int64_t n, int64_t at) {
        if (n) MRC_HIP(h, hipMemcpyAsync(out[r] + at, buf, (size_t)n, hipMemcpyDeviceToHost, st));
        MRC_HIP(h, hipStreamSynchronize(st));            // (the next slab reuses the buffer)
        return (int)MRC_OK;
    }, after);
    if (rc == MRC_ERR_NOMEM)
        return fail(h, MRC_ERR_NOMEM, std::string(who) + (c.rates ? ": an out_cap too small (see total_bytes)"
                                                                  : ": out_cap too small (see total_bytes; mrc_chain_fetch_output)"));
    return rc;
}

}  // namespace

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
    return chained_slabs(h, c, &out_cap, out, [](int, uint8_t*, int64_t, int64_t) { return (int)MRC_OK; }, NoAfter{});
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
    int rc = chained_slabs(h, c, out_cap, nullptr, [out, st, h](int r, uint8_t* buf, int64_t n, int64_t at) {
        if (n) MRC_HIP(h, hipMemcpyAsync(out[r] + at, buf, (size_t)n, hipMemcpyDeviceToDevice, st));
        return (int)MRC_OK;
    }, NoAfter{});
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

// ---- encode to a target noise-to-mask ratio (include/mrc_hip.h: mrc_encode_chained_target_nmr_pac) -----------------------
// A rate ladder whose rungs are measured where they are made.  Every slab runs as a ladder slab (chained_core) and, while
// the scan's planes are still in device memory, target_nmr_slab measures each (block, output channel) of each rung against
// the source: launch_mdct and launch_smr exactly as mrc_pac_nmr calls them (mono, explicit offsets, the generic mode that
// writes thresholds, MRC_OPT_EXACT_SPREAD honoured) on the stream's own rows and on Close()'s gathered blocks, then
// nmr_rungs_kernel.  The streams of a slab -- or, for a stream cut into time slabs, the stream once its last slab ran -- are
// DECIDED: nmr_file_kernel over [rungs x streams] pseudo-files, one small copy back, the dB values and the rule on the host,
// and the chosen files gathered behind each other in TargetBufs::sel.  The caller's buffer receives that run alone.
// (The source analysis is run again rather than taken from phase A's lines: a joint group keeps L, R, M, S rows of one block
// side by side and comes from the four-signal kernels, mrc_pac_nmr's X from the one-signal kernels on explicit offsets; the
// numbers must be mrc_pac_nmr's to the bit, so the calls are the same calls.)
namespace {

constexpr int64_t kTargetBatch = 16384;   // blocks of one shape analysed at a time: X and T of a batch stay below 512 MB

struct TargetSeg { int r; int64_t off, n; };   // bytes of rung r of one time slab in TargetBufs::keep

struct ChainNmr {
    std::vector<Slab> plan;          // the call's slabs (chained_slabs' own plan) ...
    size_t slab = 0;                 // ... and the one that runs
    const int64_t* blockStart = nullptr;   // the caller's
    int64_t unitChunks = 0;          // chunks of one rung of the streams being decided: the stride of stat's rows
    std::vector<int64_t> flushOffs;  // Close()'s blocks in flushPcm (a queued copy reads it)
    std::vector<TargetSeg> segs;
    int64_t keepUsed = 0, selUsed = 0;
    double msNmr = 0, msGather = 0;
};

// room for `need` more bytes behind the `used` bytes a buffer holds, which stay
int grow_kept(mrc_handle* h, DevBuf& b, int64_t used, int64_t need, hipStream_t st) {
    if ((size_t)(used + need) <= b.cap) return MRC_OK;
    DevBuf bigger;
    MRC_HIP(h, bigger.reserve(std::max<size_t>(2 * b.cap, (size_t)(used + need))));
    hipError_t e = hipSuccess;
    if (used) e = hipMemcpyAsync(bigger.p, b.p, (size_t)used, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { bigger.release(); return hip_fail(h, e, "mrc_encode_chained_target_nmr_pac: growing a device buffer"); }
    b.release();
    b = bigger;
    return MRC_OK;
}

int64_t stream_chunks(const ChainCall& c, const int64_t* block_start, int64_t s) {   // blocks + Close(), a chunk per channel
    return c.nch() * (block_start[s + 1] - block_start[s] + 1);
}

int target_nmr_slab(mrc_handle* h, const ChainCall& c, const ChainSchedule& q, const int64_t* count, hipStream_t st) {
    ChainNmr& N = *c.nmr;
    ChainBufs& C = h->chain;
    TargetBufs& T = h->target;
    const Slab& sl = N.plan[N.slab];
    const int R = c.n_rates, nch = c.nch(), L = h->cfg.n_mdct_lines;
    int64_t chunkBase = 0;
    if (sl.first) {                                      // the first slab of the streams decided together: their stat rows
        N.unitChunks = sl.timeSlab ? stream_chunks(c, N.blockStart, sl.s0) : c.n_chunks();
        MRC_HIP(h, T.stat.reserve((size_t)(R * N.unitChunks) * 2 * sizeof(double)));
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
    MRC_HIP(h, hipEventRecord(T.ev[0], st));
    for (int g = 0; g < q.nGroups; ++g) {
        if (!count[g]) continue;
        const DevShape& S = q.hs[g]->dev;
        const int joint = (g == 4 || nch == 1) ? 0 : 1, nOut = joint ? 2 : 1, M = S.halfN;
        for (int64_t k0 = 0; k0 < count[g]; k0 += kTargetBatch) {
            const int64_t n = std::min<int64_t>(kTargetBatch, count[g] - k0);
            const int64_t* offs = (g == 4 ? T.flushOffs.as<int64_t>() : C.g[g].offsets.as<int64_t>()) + k0;
            for (int ch = 0; ch < nOut; ++ch) {
                const void* src = g == 4 ? C.flushPcm.p : (ch ? c.pcm_right : c.pcm_left);
                double* X = T.lines.as<double>() + ch * n * M;
                int* os = T.oscale.as<int>() + ch * n;
                MRC_HIP(h, launch_mdct(S, n, src, nullptr, kSampleI16, 0, offs, true, X, os, st));
                MRC_HIP(h, launch_smr(S, n, src, nullptr, kSampleI16, 0, offs, X, os, T.smr.as<double>() + ch * n * kMaxBands,
                                      T.thresh.as<double>() + ch * n * M, nullptr, nullptr, h->exactSpread, st));
            }
            MRC_HIP(h, launch_nmr_rungs(S, R, joint, n, k0, C.groupDesc.as<ChainGroupDev>(), g,
                                        C.g[g].chunkMap.as<long long>() + k0 * nOut, T.lines.as<double>(), T.thresh.as<double>(),
                                        T.stat.as<double>(), N.unitChunks, chunkBase, st));
        }
    }
    MRC_HIP(h, hipEventRecord(T.ev[1], st));
    return MRC_OK;
}

int target_nmr_time(mrc_handle* h, const ChainCall& c) {
    float ms = 0.f;
    MRC_HIP(h, hipEventElapsedTime(&ms, h->target.ev[0], h->target.ev[1]));
    c.nmr->msNmr += ms;
    return MRC_OK;
}

// what a call returns beside the bytes
struct TargetOut {
    double target;
    int64_t* stream_byte_offset; int32_t *chosen, *met;
    double *nmr_total_db, *nmr_max_db; int64_t *disturbed_blocks, *n_blocks;
};

// The streams sl.s0 .. sl.s0 + sl.ns - 1 have all their entries in stat and all their bytes packed: reduce, decide, gather.
// Whole-stream slab: rung r's bytes of stream s are at buf + base[r] + sOff[r][s]; time slabs: in the segments of `keep`.
int target_decide(mrc_handle* h, const ChainCall& c, ChainNmr& N, const TargetOut& o, const Slab& sl, const int64_t* sOff,
                  const int64_t* base, const uint8_t* buf, hipStream_t st) {
    TargetBufs& T = h->target;
    const int R = c.n_rates, nch = c.nch(), L = h->cfg.n_mdct_lines;
    const int64_t nS = c.n_streams, ns = sl.ns, nFiles = R * ns;
    // pseudo-file (r, s): entries [r * unitChunks + first chunk of s, ...), in file order
    std::vector<long long> tab((size_t)nFiles + 1 + (size_t)(nFiles + 1) / 2 + 1);
    int* nchTab = (int*)(tab.data() + nFiles + 1);
    for (int r = 0; r < R; ++r) {
        int64_t first = 0;
        for (int64_t s = 0; s < ns; ++s) {
            tab[(size_t)(r * ns + s)] = r * N.unitChunks + first;
            nchTab[r * ns + s] = nch;
            first += stream_chunks(c, N.blockStart, sl.s0 + s);
        }
    }
    tab[(size_t)nFiles] = R * N.unitChunks;
    std::vector<double> fileOut((size_t)nFiles * 4);
    MRC_HIP(h, T.fileTab.reserve(tab.size() * sizeof(long long)));
    MRC_HIP(h, T.fileOut.reserve(fileOut.size() * sizeof(double)));
    DrainGuard guard{{st}};                              // (behind the vectors queued copies read and write)
    MRC_HIP(h, hipMemcpyAsync(T.fileTab.p, tab.data(), tab.size() * sizeof(long long), hipMemcpyHostToDevice, st));
    MRC_HIP(h, hipEventRecord(T.ev[2], st));
    MRC_HIP(h, launch_nmr_file(nFiles, T.fileTab.as<long long>(), (const int*)(T.fileTab.as<long long>() + nFiles + 1),
                               T.stat.as<double>(), T.fileOut.as<double>(), st));
    MRC_HIP(h, hipEventRecord(T.ev[3], st));
    MRC_HIP(h, hipMemcpyAsync(fileOut.data(), T.fileOut.p, fileOut.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    MRC_HIP(h, hipStreamSynchronize(st));
    // ---- the dB values as mrc_pac_nmr forms them, and the rule
    const double ninf = -std::numeric_limits<double>::infinity();
    std::vector<long long> span((size_t)ns * 3);
    int64_t maxLen = 0, selNeed = 0;
    for (int64_t s = 0; s < ns; ++s) {
        const int64_t gs = sl.s0 + s;
        int64_t weight = (int64_t)L * nch;                                      // Close()'s block
        for (int64_t i = N.blockStart[gs]; i < N.blockStart[gs + 1]; ++i) weight += (int64_t)c.block_b[i] * nch;
        o.n_blocks[gs] = N.blockStart[gs + 1] - N.blockStart[gs] + 1;
        int pick = R - 1, met = 0;
        for (int r = R - 1; r >= 0; --r) {
            const double* f = fileOut.data() + 4 * (r * ns + s);
            const double mean = weight > 0 ? f[1] / (double)weight : 0.0;
            const double total = mean > 0.0 ? 10.0 * std::log10(mean) : ninf;
            o.nmr_max_db[r * nS + gs] = f[0] > 0.0 ? 10.0 * std::log10(f[0]) : ninf;
            o.nmr_total_db[r * nS + gs] = total;
            o.disturbed_blocks[r * nS + gs] = (int64_t)f[2];
            if (total <= o.target) { pick = r; met = 1; }                       // (descending: the smallest r that meets it stays)
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
    float a = 0.f, b = 0.f;
    MRC_HIP(h, hipEventElapsedTime(&a, T.ev[2], T.ev[3]));
    MRC_HIP(h, hipEventElapsedTime(&b, T.ev[4], T.ev[5]));
    N.msNmr += a;
    N.msGather += b;
    return MRC_OK;
}

// the block layout a call that measures its own output needs (the NMR positions blocks by their offsets; whole files)
int layout_check(mrc_handle* h, const std::string& w, int64_t n_streams, const int64_t* block_start, const int64_t* block_offset,
                 const int32_t* block_a, const int32_t* block_b);

// the refusals of include/mrc_hip.h, before any device work
int target_check(mrc_handle* h, const std::string& w, int n_rates, const double* rates, double target, int64_t n_streams,
                 const void* pcm_left, int64_t stream_stride, const int64_t* block_start, const int64_t* block_offset,
                 const int32_t* block_a, const int32_t* block_b, const uint32_t* num_samples, const uint8_t* out, int64_t out_cap,
                 const TargetOut& o, const int64_t* total_bytes) {
    if (!h) return MRC_ERR_INVALID;
    if (n_rates < 1 || n_rates > MRC_MAX_RATES) return fail(h, MRC_ERR_INVALID, w + ": n_rates must lie in 1..MRC_MAX_RATES (16)");
    if (!rates) return fail(h, MRC_ERR_INVALID, w + ": target_bits_per_sample must not be NULL");
    for (int r = 0; r < n_rates; ++r) {
        if (!std::isfinite(rates[r]) || !(rates[r] > 0.0) || rates[r] > 64.0)
            return fail(h, MRC_ERR_INVALID, w + ": target_bits_per_sample[" + std::to_string(r) + "] must be finite and in (0, 64]");
        if (r && !(rates[r] > rates[r - 1]))
            return fail(h, MRC_ERR_INVALID, w + ": target_bits_per_sample must be strictly ascending (entry " + std::to_string(r) + " is not)");
    }
    if (std::isnan(target)) return fail(h, MRC_ERR_INVALID, w + ": target_nmr_total_db is NaN");
    if (!num_samples) return fail(h, MRC_ERR_INVALID, w + ": num_samples must not be NULL (whole files only)");
    if (h->sensOn)
        return fail(h, MRC_ERR_INVALID, w + ": MRC_OPT_SENSITIVITY is on (the certificate covers one rate: encode each rate on its own)");
    if (n_streams < 0 || !pcm_left || stream_stride <= 0 || !block_start || !block_offset || !block_a || !block_b || !out ||
        out_cap < 0 || !o.stream_byte_offset || !o.chosen || !o.met || !o.nmr_total_db || !o.nmr_max_db || !o.disturbed_blocks ||
        !o.n_blocks || !total_bytes)
        return fail(h, MRC_ERR_INVALID, w + ": bad argument (a NULL pointer, a negative count or capacity)");
    return layout_check(h, w, n_streams, block_start, block_offset, block_a, block_b);
}

int layout_check(mrc_handle* h, const std::string& w, int64_t n_streams, const int64_t* block_start, const int64_t* block_offset,
                 const int32_t* block_a, const int32_t* block_b) {
    const int L = h->cfg.n_mdct_lines;
    for (int64_t s = 0; s < n_streams; ++s) {
        const int64_t i0 = block_start[s], i1 = block_start[s + 1];
        const std::string which = w + ": stream " + std::to_string(s);
        if (i1 <= i0) return fail(h, MRC_ERR_INVALID, which + ": block_start gives it no block");
        if (block_a[i0] != L)
            return fail(h, MRC_ERR_INVALID, which + ": block_a of its first block must be n_mdct_lines (the zero prior hop)");
        int64_t sum = 0;
        for (int64_t i = i0; i < i1; ++i) {
            if (block_offset[i] != sum)
                return fail(h, MRC_ERR_INVALID, which + ": block_offset[" + std::to_string(i) + "] must be the sum of block_a of the "
                                                "stream's earlier blocks (" + std::to_string(sum) + "): the NMR positions blocks by it");
            sum += block_a[i];
        }
        if (block_b[i1 - 1] != L)
            return fail(h, MRC_ERR_INVALID, which + ": block_b of its last block must be n_mdct_lines (a stream must end with a long "
                                            "block: the reference's Close() assumes it, pacfileThem.py:973-984)");
    }
    return MRC_OK;
}

// pcm_left / pcm_right in device memory; the chosen bytes end in TargetBufs::sel and, if they fit, in out (host or device)
int chained_target(mrc_handle* h, const std::string& w, ChainCall c, const TargetOut& o, uint8_t* out, int64_t out_cap,
                   bool outOnHost, int64_t* total_bytes, hipStream_t st) {
    const int R = c.n_rates;
    const int64_t nS = c.n_streams;
    ChainBufs& C = h->chain;
    TargetBufs& T = h->target;
    for (auto& e : T.ev) if (!e) MRC_HIP(h, hipEventCreate(&e));
    ChainNmr N;
    N.blockStart = c.block_start;
    N.plan = plan_slabs(nS, c.block_start, slab_cap(h, R, c.nch()));
    std::vector<int64_t> sOff((size_t)R * (nS + 1)), totals((size_t)R), caps((size_t)R, std::numeric_limits<int64_t>::max() / 4);
    c.stream_byte_offset = sOff.data();
    c.total_bytes = totals.data();
    c.nmr = &N;
    *total_bytes = 0;
    o.stream_byte_offset[0] = 0;
    int rc = chained_slabs(h, c, caps.data(), nullptr,
        [&](int r, uint8_t* buf, int64_t n, int64_t) {
            if (!N.plan[N.slab].timeSlab) return (int)MRC_OK;        // (whole streams: gathered from the slab's buffer)
            MRC_TRY(grow_kept(h, T.keep, N.keepUsed, std::max<int64_t>(n, 1), st));
            if (n) MRC_HIP(h, hipMemcpyAsync(T.keep.as<uint8_t>() + N.keepUsed, buf, (size_t)n, hipMemcpyDeviceToDevice, st));
            N.segs.push_back(TargetSeg{r, N.keepUsed, n});
            N.keepUsed += n;
            return (int)MRC_OK;
        },
        [&](const Slab& sl, const int64_t* slabOff, const int64_t* base, const uint8_t* buf) {
            if (sl.last) MRC_TRY(target_decide(h, c, N, o, sl, slabOff, base, buf, st));
            ++N.slab;
            return (int)MRC_OK;
        });
    T.ms[0] = h->chainMs[0]; T.ms[1] = h->chainMs[1]; T.ms[2] = N.msNmr; T.ms[3] = h->chainMs[2] + N.msGather;
    if (rc != MRC_OK) return rc;
    const int64_t total = N.selUsed;
    *total_bytes = total;
    o.stream_byte_offset[nS] = total;
    C.lastTotal = total;                                 // (mrc_chain_fetch_output: the chosen bytes, whatever out_cap was)
    C.lastSrc = T.sel.p;
    if (total > out_cap) return fail(h, MRC_ERR_NOMEM, w + ": out_cap too small (see total_bytes; mrc_chain_fetch_output)");
    if (total) MRC_HIP(h, hipMemcpyAsync(out, T.sel.p, (size_t)total, outOnHost ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
    MRC_HIP(h, hipStreamSynchronize(st));
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
    MRC_TRY(target_check(h, __func__, n_rates, target_bits_per_sample, target_nmr_total_db, n_streams, pcm_left, stream_stride,
                         block_start, block_offset, block_a, block_b, num_samples, out, out_cap, o, total_bytes));
    ChainCall c{n_rates, target_bits_per_sample, n_streams, pcm_left, pcm_right, MRC_SAMPLES_PCM16, stream_stride, block_start,
                block_offset, block_a, block_b, nullptr, use_huffman, 1, num_samples, nullptr, nullptr, nullptr, nullptr, nullptr,
                nullptr};
    h->chain.lastTotal = -1;
    h->chain.lastSrc = nullptr;
    MRC_HIP(h, hipSetDevice(h->device));
    MRC_TRY(stage_pcm(h, c));
    c.pcm_left = h->chain.pcmL.p;
    if (c.pcm_right) c.pcm_right = h->chain.pcmR.p;
    return chained_target(h, __func__, c, o, out, out_cap, true, total_bytes, h->stream);
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
    MRC_TRY(target_check(h, __func__, n_rates, target_bits_per_sample, target_nmr_total_db, n_streams, pcm_left, stream_stride,
                         block_start, block_offset, block_a, block_b, num_samples, out, out_cap, o, total_bytes));
    const ChainCall c{n_rates, target_bits_per_sample, n_streams, pcm_left, pcm_right, MRC_SAMPLES_PCM16, stream_stride, block_start,
                      block_offset, block_a, block_b, nullptr, use_huffman, 1, num_samples, nullptr, nullptr, nullptr, nullptr,
                      nullptr, stream};
    h->chain.lastTotal = -1;
    h->chain.lastSrc = nullptr;
    MRC_HIP(h, hipSetDevice(h->device));
    return chained_target(h, __func__, c, o, out, out_cap, false, total_bytes, pick_stream(h, stream));
}

int mrc_get_target_ms(mrc_handle* h, double* ms) {
    if (!h || !ms) return MRC_ERR_INVALID;
    for (int i = 0; i < 4; ++i) ms[i] = h->target.ms[i];
    return MRC_OK;
}

}  // extern "C"

// ---- constant-quality VBR (include/mrc_hip.h: mrc_encode_vbr_nmr_pac; the rule: DESIGN.md section 12) ---------------------
// A one-rate chained call without a budget.  chained_core runs phase A up to the M/S switch (no SMRs, no event lists), and
// where the serial scan would run, vbr_slab analyses the source exactly as target_nmr_slab does -- launch_mdct and launch_smr
// in the mode that writes thresholds, mono, explicit offsets, MRC_OPT_EXACT_SPREAD honoured -- and vbr_alloc_kernel writes
// the planes the packer reads, the entries' statistics and the capped bands.  The packer chooses the Huffman tables.  The
// streams of a slab -- a stream cut into time slabs: once its last slab ran -- are reduced by nmr_file_kernel (vbr_decide).
// The bytes travel as the one-rate chained call's do.
// mrc_encode_vbr_size_pac: the same slab with vbr_profile_kernel in vbr_alloc_kernel's place and
// vbr_size_search behind it; everything after it -- pack, headers, vbr_decide -- is the VBR call's.
namespace {

// mrc_encode_vbr_size_pac: the grid, the size limits and the per-stream results of the search, all the caller's
struct VbrSize {
    double lo, step; int n; const int64_t* target;
    int32_t* chosen; double *chosen_db, *ceiling_ratio; int32_t *met, *probes, *probe_index; int64_t* probe_bytes;
    double db(int i) const { return lo + (double)i * step; }
};

struct ChainVbr {
    std::vector<Slab> plan;          // the call's slabs (chained_slabs' own plan) ...
    size_t slab = 0;                 // ... and the one that runs
    const int64_t* blockStart = nullptr;   // the caller's
    double ceiling = 0.0;            // c, the linear ratio
    int64_t unitChunks = 0;          // chunks of the streams being decided
    std::vector<int64_t> flushOffs;  // Close()'s blocks in flushPcm (a queued copy reads it)
    double msAlloc = 0;
    const VbrSize* size = nullptr;   // mrc_encode_vbr_size_pac: the slab records the walk and searches the grid (vbr_size_search)
    double msProbe = 0, msPick = 0;
};

struct VbrOut { int64_t *capped_bands, *coded_bits; double *nmr_total_db, *nmr_max_db; int64_t *disturbed_blocks, *n_blocks; };

// The search of one slab's streams (include/mrc_hip.h states the rule): the record of every block is in VbrBufs::prof.  A
// probe: vbr_pick_kernel at each stream's ceiling, the packer's plan (pricing only), the streams' file sizes, one copy back;
// the host moves every unfinished stream's interval.  At most MRC_MAX_PROBES rounds whatever the number of streams.  It
// leaves the planes, T.stat and V.capped at the chosen ceilings, as vbr_alloc_kernel would.
int vbr_size_search(mrc_handle* h, const ChainCall& c, const ChainSchedule& q, const int64_t* count, hipStream_t st) {
    ChainVbr& N = *c.vbr;
    const VbrSize& Z = *N.size;
    ChainBufs& C = h->chain;
    TargetBufs& T = h->target;
    VbrBufs& V = h->vbr;
    const int nch = c.nch();
    const int64_t nS = c.n_streams, nChunks = c.n_chunks(), s0 = N.plan[N.slab].s0;
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

int vbr_slab(mrc_handle* h, const ChainCall& c, const ChainSchedule& q, const int64_t* count, hipStream_t st) {
    ChainVbr& N = *c.vbr;
    ChainBufs& C = h->chain;
    TargetBufs& T = h->target;
    VbrBufs& V = h->vbr;
    const Slab& sl = N.plan[N.slab];
    const int nch = c.nch(), L = h->cfg.n_mdct_lines;
    int64_t chunkBase = 0;
    if (sl.first) {                                      // the first slab of the streams decided together: their rows
        N.unitChunks = sl.timeSlab ? stream_chunks(c, N.blockStart, sl.s0) : c.n_chunks();
        MRC_HIP(h, T.stat.reserve((size_t)N.unitChunks * 2 * sizeof(double)));
        MRC_HIP(h, V.capped.reserve((size_t)N.unitChunks * sizeof(int)));
    } else chunkBase = nch * (sl.i0 - N.blockStart[sl.s0]);
    size_t rowBytes = 0, rows = 0, launches = 0;
    for (int g = 0; g < q.nGroups; ++g) {
        const int nOut = (g == 4 || nch == 1) ? 1 : 2;
        const size_t n = (size_t)std::min<int64_t>(count[g], kTargetBatch) * nOut;
        rows = std::max(rows, n);
        rowBytes = std::max(rowBytes, n * q.hs[g]->dev.halfN * sizeof(double));
        launches += (size_t)((count[g] + kTargetBatch - 1) / kTargetBatch);
    }
    MRC_HIP(h, T.lines.reserve(std::max<size_t>(rowBytes, 256)));
    MRC_HIP(h, T.thresh.reserve(std::max<size_t>(rowBytes, 256)));
    MRC_HIP(h, T.oscale.reserve(std::max<size_t>(rows * sizeof(int), 256)));
    MRC_HIP(h, T.smr.reserve(std::max<size_t>(rows * kMaxBands * sizeof(double), 256)));
    while (V.ev.size() < 2 * launches) {
        hipEvent_t e = nullptr;
        MRC_HIP(h, hipEventCreate(&e));
        V.ev.push_back(e);
    }
    V.evUsed = 0;
    if (N.size) {                                        // the record of every block of the slab, group by group
        for (auto& e : V.evSize) if (!e) MRC_HIP(h, hipEventCreate(&e));
        for (int g = 0; g < q.nGroups; ++g) {
            const int joint = (g == 4 || nch == 1) ? 0 : 1;
            MRC_HIP(h, V.prof[g].reserve(std::max<size_t>((size_t)count[g] * vbr_profile_bytes(q.hs[g]->dev, joint), 256)));
            if (joint) MRC_HIP(h, V.profPick[g].reserve(std::max<size_t>((size_t)count[g] * q.hs[g]->dev.nBands * sizeof(unsigned), 256)));
        }
    }
    if (c.with_flush) {
        N.flushOffs.resize((size_t)count[4]);
        for (int64_t k = 0; k < count[4]; ++k) N.flushOffs[(size_t)k] = k * 2 * (int64_t)L;
        MRC_HIP(h, T.flushOffs.reserve(std::max<size_t>(N.flushOffs.size() * sizeof(int64_t), 256)));
        if (count[4])
            MRC_HIP(h, hipMemcpyAsync(T.flushOffs.p, N.flushOffs.data(), N.flushOffs.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    }
    for (int g = 0; g < q.nGroups; ++g) {
        if (!count[g]) continue;
        const DevShape& S = q.hs[g]->dev;
        const int joint = (g == 4 || nch == 1) ? 0 : 1, nOut = joint ? 2 : 1, M = S.halfN;
        ChainGroupBufs& B = C.g[g];
        for (int64_t k0 = 0; k0 < count[g]; k0 += kTargetBatch) {
            const int64_t n = std::min<int64_t>(kTargetBatch, count[g] - k0);
            const int64_t* offs = (g == 4 ? T.flushOffs.as<int64_t>() : B.offsets.as<int64_t>()) + k0;
            for (int ch = 0; ch < nOut; ++ch) {
                const void* src = g == 4 ? C.flushPcm.p : (ch ? c.pcm_right : c.pcm_left);
                double* X = T.lines.as<double>() + ch * n * M;
                int* os = T.oscale.as<int>() + ch * n;
                MRC_HIP(h, launch_mdct(S, n, src, nullptr, kSampleI16, 0, offs, true, X, os, st));
                MRC_HIP(h, launch_smr(S, n, src, nullptr, kSampleI16, 0, offs, X, os, T.smr.as<double>() + ch * n * kMaxBands,
                                      T.thresh.as<double>() + ch * n * M, nullptr, nullptr, h->exactSpread, st));
            }
            MRC_HIP(h, hipEventRecord(V.ev[V.evUsed++], st));
            if (N.size)
                MRC_HIP(h, launch_vbr_profile(S, joint, n, k0, B.lines.as<double>(), B.oscale.as<int>(),
                                              joint ? B.ms.as<int>() : nullptr, T.lines.as<double>(), T.thresh.as<double>(),
                                              V.prof[g].as<double>(), joint ? V.profPick[g].as<unsigned>() : nullptr, st));
            else
                MRC_HIP(h, launch_vbr_alloc(S, joint, n, k0, N.ceiling, B.lines.as<double>(), B.oscale.as<int>(),
                                            joint ? B.ms.as<int>() : nullptr, B.bitAlloc.as<int>(), B.scaleFactor.as<int>(),
                                            B.mant.as<unsigned short>(), B.chunkMap.as<long long>() + k0 * nOut, T.lines.as<double>(),
                                            T.thresh.as<double>(), T.stat.as<double>(), V.capped.as<int>(), chunkBase, st));
            MRC_HIP(h, hipEventRecord(V.ev[V.evUsed++], st));
        }
    }
    if (N.size) MRC_TRY(vbr_size_search(h, c, q, count, st));
    return MRC_OK;
}

int vbr_time(mrc_handle* h, const ChainCall& c) {
    VbrBufs& V = h->vbr;
    for (size_t i = 0; i + 1 < V.evUsed; i += 2) {
        float ms = 0.f;
        MRC_HIP(h, hipEventElapsedTime(&ms, V.ev[i], V.ev[i + 1]));
        c.vbr->msAlloc += ms;
    }
    if (c.vbr->size) {
        float a = 0.f, b = 0.f;
        MRC_HIP(h, hipEventElapsedTime(&a, V.evSize[0], V.evSize[1]));
        MRC_HIP(h, hipEventElapsedTime(&b, V.evSize[1], V.evSize[2]));
        c.vbr->msProbe += a;
        c.vbr->msPick += b;
    }
    return MRC_OK;
}

// The streams sl.s0 .. sl.s0 + sl.ns - 1 have all their entries in stat: the file reduction, the dB values as mrc_pac_nmr
// forms them, the capped bands.
int vbr_decide(mrc_handle* h, const ChainCall& c, ChainVbr& N, const VbrOut& o, const Slab& sl, hipStream_t st) {
    TargetBufs& T = h->target;
    const int nch = c.nch(), L = h->cfg.n_mdct_lines;
    const int64_t ns = sl.ns;
    std::vector<long long> tab((size_t)ns + 1 + (size_t)(ns + 1) / 2 + 1);
    int* nchTab = (int*)(tab.data() + ns + 1);
    int64_t first = 0;
    for (int64_t s = 0; s < ns; ++s) {
        tab[(size_t)s] = first;
        nchTab[s] = nch;
        first += stream_chunks(c, N.blockStart, sl.s0 + s);
    }
    tab[(size_t)ns] = first;
    std::vector<double> fileOut((size_t)ns * 4);
    std::vector<int> capped((size_t)first);
    MRC_HIP(h, T.fileTab.reserve(tab.size() * sizeof(long long)));
    MRC_HIP(h, T.fileOut.reserve(fileOut.size() * sizeof(double)));
    DrainGuard guard{{st}};                              // (behind the vectors queued copies read and write)
    MRC_HIP(h, hipMemcpyAsync(T.fileTab.p, tab.data(), tab.size() * sizeof(long long), hipMemcpyHostToDevice, st));
    MRC_HIP(h, launch_nmr_file(ns, T.fileTab.as<long long>(), (const int*)(T.fileTab.as<long long>() + ns + 1),
                               T.stat.as<double>(), T.fileOut.as<double>(), st));
    MRC_HIP(h, hipMemcpyAsync(fileOut.data(), T.fileOut.p, fileOut.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    MRC_HIP(h, hipMemcpyAsync(capped.data(), h->vbr.capped.p, capped.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    MRC_HIP(h, hipStreamSynchronize(st));
    const double ninf = -std::numeric_limits<double>::infinity();
    for (int64_t s = 0; s < ns; ++s) {
        const int64_t gs = sl.s0 + s;
        int64_t weight = (int64_t)L * nch;                                      // Close()'s block
        for (int64_t i = N.blockStart[gs]; i < N.blockStart[gs + 1]; ++i) weight += (int64_t)c.block_b[i] * nch;
        const double* f = fileOut.data() + 4 * s;
        const double mean = weight > 0 ? f[1] / (double)weight : 0.0;
        o.n_blocks[gs] = N.blockStart[gs + 1] - N.blockStart[gs] + 1;
        o.nmr_total_db[gs] = mean > 0.0 ? 10.0 * std::log10(mean) : ninf;
        o.nmr_max_db[gs] = f[0] > 0.0 ? 10.0 * std::log10(f[0]) : ninf;
        o.disturbed_blocks[gs] = (int64_t)f[2];
        int64_t cap = 0;
        for (long long k = tab[(size_t)s]; k < tab[(size_t)s + 1]; ++k) cap += capped[(size_t)k];
        o.capped_bands[gs] = cap;
    }
    return MRC_OK;
}

// the refusals of include/mrc_hip.h, before any device work
int vbr_check(mrc_handle* h, const std::string& w, double ceiling_db, int64_t n_streams, const void* pcm_left, int64_t stream_stride,
              const int64_t* block_start, const int64_t* block_offset, const int32_t* block_a, const int32_t* block_b,
              const uint32_t* num_samples, const uint8_t* out, int64_t out_cap, const int64_t* stream_byte_offset,
              const double* ceiling_ratio, const VbrOut& o, const int64_t* total_bytes) {
    if (!h) return MRC_ERR_INVALID;
    if (std::isnan(ceiling_db)) return fail(h, MRC_ERR_INVALID, w + ": ceiling_db is NaN");
    if (!num_samples) return fail(h, MRC_ERR_INVALID, w + ": num_samples must not be NULL (whole files only)");
    if (h->sensOn)
        return fail(h, MRC_ERR_INVALID, w + ": MRC_OPT_SENSITIVITY is on (the certificate covers the budgeted allocation, not this one)");
    if (n_streams < 0 || !pcm_left || stream_stride <= 0 || !block_start || !block_offset || !block_a || !block_b || !out ||
        out_cap < 0 || !stream_byte_offset || !ceiling_ratio || !o.capped_bands || !o.coded_bits || !o.nmr_total_db ||
        !o.nmr_max_db || !o.disturbed_blocks || !o.n_blocks || !total_bytes)
        return fail(h, MRC_ERR_INVALID, w + ": bad argument (a NULL pointer, a negative count or capacity)");
    return layout_check(h, w, n_streams, block_start, block_offset, block_a, block_b);
}

// behind the slabs: the sizes as payload bits, the times
int vbr_finish(mrc_handle* h, const ChainCall& c, const ChainVbr& N, const VbrOut& o) {
    const int nch = c.nch();
    uint8_t one[256];
    int64_t hdrLen = 0;
    if (c.n_streams && (mrc_pac_header(&h->cfg, nch, c.num_samples[0], one, sizeof(one), &hdrLen) != MRC_OK))
        return fail(h, MRC_ERR_INVALID, "mrc_encode_vbr_nmr_pac: mrc_pac_header failed");
    for (int64_t s = 0; s < c.n_streams; ++s)            // a chunk: a 4-byte length and its payload
        o.coded_bits[s] = 8 * (c.stream_byte_offset[s + 1] - c.stream_byte_offset[s] - hdrLen - 4 * stream_chunks(c, N.blockStart, s));
    VbrBufs& V = h->vbr;
    V.ms[0] = h->chainMs[0] + h->chainMs[1] - N.msAlloc;
    V.ms[1] = N.msAlloc;
    V.ms[2] = h->chainMs[2];
    V.ms[3] = h->chainMs[3];
    if (N.size) {
        V.sizeMs[0] = V.ms[0] - N.msProbe - N.msPick;
        V.sizeMs[1] = N.msAlloc;
        V.sizeMs[2] = N.msProbe;
        V.sizeMs[3] = N.msPick + h->chainMs[2];
        V.sizeMs[4] = h->chainMs[3];
    }
    return MRC_OK;
}

// mrc_encode_vbr_size_pac's own refusals behind vbr_check's, and the trace cleared
int vbr_size_check(mrc_handle* h, const std::string& w, const VbrSize& Z, int64_t n_streams, const int64_t* block_start, int nch) {
    if (!std::isfinite(Z.lo)) return fail(h, MRC_ERR_INVALID, w + ": ceiling_lo_db must be finite");
    if (!std::isfinite(Z.step) || !(Z.step > 0.0)) return fail(h, MRC_ERR_INVALID, w + ": ceiling_step_db must be finite and > 0");
    if (Z.n < 1 || Z.n > MRC_MAX_CEILINGS) return fail(h, MRC_ERR_INVALID, w + ": n_ceilings must lie in 1..MRC_MAX_CEILINGS (256)");
    if (!Z.target) return fail(h, MRC_ERR_INVALID, w + ": target_bytes must not be NULL");
    if (!Z.chosen || !Z.chosen_db || !Z.met || !Z.probes)
        return fail(h, MRC_ERR_INVALID, w + ": chosen, chosen_db, met and probes must not be NULL");
    const int64_t cap = vbr_size_slab_blocks(h, nch);
    for (int64_t s = 0; s < n_streams; ++s) {
        if (Z.target[s] < 0) return fail(h, MRC_ERR_INVALID, w + ": target_bytes[" + std::to_string(s) + "] is negative");
        if (block_start[s + 1] - block_start[s] > cap)
            return fail(h, MRC_ERR_INVALID, w + ": stream " + std::to_string(s) + " has " + std::to_string(block_start[s + 1] - block_start[s]) +
                                            " blocks, a slab of this call holds " + std::to_string(cap) + " (MRC_OPT_CHAIN_SLAB_BLOCKS): "
                                            "the search needs all blocks of a stream resident at once");
    }
    for (int64_t s = 0; s < n_streams; ++s) {
        Z.probes[s] = 0;
        for (int p = 0; p < MRC_MAX_PROBES; ++p) {
            if (Z.probe_index) Z.probe_index[s * MRC_MAX_PROBES + p] = -1;
            if (Z.probe_bytes) Z.probe_bytes[s * MRC_MAX_PROBES + p] = -1;
        }
    }
    return MRC_OK;
}

// both entry points: pcm and out in host memory (the PCM staged, the bytes copied back slab by slab) or on the device
int vbr_size_call(mrc_handle* h, const char* who, const VbrSize& Z, ChainCall c, const VbrOut& o, uint8_t* out, int64_t out_cap,
                  bool onHost) {
    MRC_TRY(vbr_check(h, who, 0.0, c.n_streams, c.pcm_left, c.stream_stride, c.block_start, c.block_offset, c.block_a, c.block_b,
                      c.num_samples, out, out_cap, c.stream_byte_offset, Z.ceiling_ratio, o, c.total_bytes));
    MRC_TRY(vbr_size_check(h, who, Z, c.n_streams, c.block_start, c.nch()));
    ChainVbr N;
    N.blockStart = c.block_start;
    N.size = &Z;
    c.slabBlocks = vbr_size_slab_blocks(h, c.nch());
    N.plan = plan_slabs(c.n_streams, c.block_start, c.slabBlocks);
    c.vbr = &N;
    hipStream_t st = onHost ? h->stream : pick_stream(h, c.stream);
    auto after = [&](const Slab& sl, const int64_t*, const int64_t*, const uint8_t*) {
        MRC_TRY(vbr_decide(h, c, N, o, sl, st));             // (whole streams only: every slab decides its own)
        ++N.slab;
        return (int)MRC_OK;
    };
    int rc;
    if (onHost) rc = chained_host(h, who, c, &out, &out_cap, after);
    else {
        MRC_TRY(check_call(h, who, c, &out, &out_cap));
        rc = chained_slabs(h, c, &out_cap, out, [](int, uint8_t*, int64_t, int64_t) { return (int)MRC_OK; }, after);
    }
    if (rc != MRC_OK && rc != MRC_ERR_NOMEM) return rc;
    const std::string err = h->error;
    MRC_TRY(vbr_finish(h, c, N, o));
    if (rc != MRC_OK) h->error = err;
    return rc;
}

}  // namespace

extern "C" {

int mrc_encode_vbr_nmr_pac(mrc_handle* h, double ceiling_db, int64_t n_streams, const int16_t* pcm_left, const int16_t* pcm_right,
                           int64_t stream_stride, const int64_t* block_start, const int64_t* block_offset,
                           const int32_t* block_a, const int32_t* block_b, int use_huffman, const uint32_t* num_samples,
                           uint8_t* out, int64_t out_cap, int64_t* stream_byte_offset, double* ceiling_ratio,
                           int64_t* capped_bands, int64_t* coded_bits, double* nmr_total_db, double* nmr_max_db,
                           int64_t* disturbed_blocks, int64_t* n_blocks, int64_t* total_bytes) {
    const VbrOut o{capped_bands, coded_bits, nmr_total_db, nmr_max_db, disturbed_blocks, n_blocks};
    MRC_TRY(vbr_check(h, __func__, ceiling_db, n_streams, pcm_left, stream_stride, block_start, block_offset, block_a, block_b,
                      num_samples, out, out_cap, stream_byte_offset, ceiling_ratio, o, total_bytes));
    ChainVbr N;
    N.blockStart = block_start;
    N.ceiling = *ceiling_ratio = std::pow(10.0, ceiling_db / 10.0);
    N.plan = plan_slabs(n_streams, block_start, slab_cap(h, 1, pcm_right ? 2 : 1));
    ChainCall c{1, nullptr, n_streams, pcm_left, pcm_right, MRC_SAMPLES_PCM16, stream_stride, block_start, block_offset,
                block_a, block_b, nullptr, use_huffman, 1, num_samples, stream_byte_offset, nullptr, nullptr, nullptr,
                total_bytes, nullptr};
    c.vbr = &N;
    hipStream_t st = h->stream;
    const int rc = chained_host(h, __func__, c, &out, &out_cap, [&](const Slab& sl, const int64_t*, const int64_t*, const uint8_t*) {
        if (sl.last) MRC_TRY(vbr_decide(h, c, N, o, sl, st));
        ++N.slab;
        return (int)MRC_OK;
    });
    if (rc != MRC_OK && rc != MRC_ERR_NOMEM) return rc;
    const std::string err = h->error;
    MRC_TRY(vbr_finish(h, c, N, o));
    if (rc != MRC_OK) h->error = err;
    return rc;
}

int mrc_dev_encode_vbr_nmr_pac(mrc_handle* h, double ceiling_db, int64_t n_streams, const int16_t* pcm_left,
                               const int16_t* pcm_right, int64_t stream_stride, const int64_t* block_start,
                               const int64_t* block_offset, const int32_t* block_a, const int32_t* block_b, int use_huffman,
                               const uint32_t* num_samples, uint8_t* out, int64_t out_cap, int64_t* stream_byte_offset,
                               double* ceiling_ratio, int64_t* capped_bands, int64_t* coded_bits, double* nmr_total_db,
                               double* nmr_max_db, int64_t* disturbed_blocks, int64_t* n_blocks, int64_t* total_bytes,
                               void* stream) {
    const VbrOut o{capped_bands, coded_bits, nmr_total_db, nmr_max_db, disturbed_blocks, n_blocks};
    MRC_TRY(vbr_check(h, __func__, ceiling_db, n_streams, pcm_left, stream_stride, block_start, block_offset, block_a, block_b,
                      num_samples, out, out_cap, stream_byte_offset, ceiling_ratio, o, total_bytes));
    ChainVbr N;
    N.blockStart = block_start;
    N.ceiling = *ceiling_ratio = std::pow(10.0, ceiling_db / 10.0);
    N.plan = plan_slabs(n_streams, block_start, slab_cap(h, 1, pcm_right ? 2 : 1));
    ChainCall c{1, nullptr, n_streams, pcm_left, pcm_right, MRC_SAMPLES_PCM16, stream_stride, block_start, block_offset,
                block_a, block_b, nullptr, use_huffman, 1, num_samples, stream_byte_offset, nullptr, nullptr, nullptr,
                total_bytes, stream};
    c.vbr = &N;
    MRC_TRY(check_call(h, __func__, c, &out, &out_cap));
    hipStream_t st = pick_stream(h, stream);
    const int rc = chained_slabs(h, c, &out_cap, out, [](int, uint8_t*, int64_t, int64_t) { return (int)MRC_OK; },
                                 [&](const Slab& sl, const int64_t*, const int64_t*, const uint8_t*) {
        if (sl.last) MRC_TRY(vbr_decide(h, c, N, o, sl, st));
        ++N.slab;
        return (int)MRC_OK;
    });
    if (rc != MRC_OK && rc != MRC_ERR_NOMEM) return rc;
    const std::string err = h->error;
    MRC_TRY(vbr_finish(h, c, N, o));
    if (rc != MRC_OK) h->error = err;
    return rc;
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
    return vbr_size_call(h, __func__, Z, c, o, out, out_cap, true);
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
    return vbr_size_call(h, __func__, Z, c, o, out, out_cap, false);
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

}  // extern "C"
