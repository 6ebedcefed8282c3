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
// No computation happens in this file.
//
// Items, in file order per stream:  stereo  one joint block (two chunks) per block shape, Close()'s two one-channel blocks
//                                           (one chunk each);
//                                   mono    one one-channel block (one chunk) per block shape, Close()'s one block.
#include "mrc_handle.hpp"

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

// One SLAB of a chained encode: all of the streams [0, n_streams) handed over, every buffer sized for exactly these blocks
// (the entry points below cut a call into slabs).  pcm_right == nullptr: mono streams.
// n_rates bit rates (rates == nullptr: one, the handle's target_bits_per_sample): phase A and the event lists once, the scan
// and the packer per (rate, stream).  Rate r's bytes are out[rate_base[r] .. + total_bytes[r]); its offsets are relative to
// rate_base[r], and every per-stream / per-item output holds n_rates rows: stream_byte_offset [R][n_streams + 1],
// item_byte_offset [R][n_items + 1], reservoir_in / reservoir_out [R][n_streams], reservoir_trace [R][n_items].
int chained_core(mrc_handle* h, int n_rates, const double* rates, int64_t n_streams, const void* pcm_left, const void* pcm_right,
                 int sample_format, int64_t stream_stride, const int64_t* block_start, const int64_t* block_offset,
                 const int32_t* block_a, const int32_t* block_b, const int32_t* reservoir_in,
                 int use_huffman, int with_flush, const uint32_t* num_samples, uint8_t* out, int64_t out_cap,
                 int64_t* stream_byte_offset, int64_t* item_byte_offset, int32_t* reservoir_out,
                 int32_t* reservoir_trace, int64_t* total_bytes, int64_t* rate_base, void* stream) {
    if (!h || n_rates < 1 || (n_rates > 1 && !rates) || n_streams < 0 || !pcm_left || stream_stride <= 0 || !block_start ||
        !block_offset || !block_a || !block_b || !out || out_cap < 0 || !stream_byte_offset || !total_bytes ||
        (sample_format != MRC_SAMPLES_F64 && sample_format != MRC_SAMPLES_PCM16))
        return fail(h, MRC_ERR_INVALID, "mrc_encode_chained: bad argument");
    const size_t sampleBytes = sample_format == MRC_SAMPLES_PCM16 ? sizeof(int16_t) : sizeof(double);
    const int R = n_rates;
    for (int r = 0; r < R; ++r) {
        total_bytes[r] = 0;
        stream_byte_offset[r * (n_streams + 1)] = 0;
        if (rate_base) rate_base[r] = 0;
    }
    if (n_streams == 0) return MRC_OK;
    const mrc_config& cfg = h->cfg;
    const int L = cfg.n_mdct_lines, Sh = cfg.n_short;
    // stereo: groups 0-3 joint (two chunks per block), Close() two one-channel items; mono: every item one channel
    const int nch = pcm_right ? 2 : 1, stereo = nch == 2;
    const int64_t b0 = block_start[0], nB = block_start[n_streams] - b0;
    if (nB < n_streams) return fail(h, MRC_ERR_INVALID, "mrc_encode_chained: every stream needs at least one block");
    // ---- the block shapes of the reference's block switching (pacfileThem.py:1192-1210); group 4: Close()'s blocks
    const int shapeA[kChainGroups] = {L, L, Sh, Sh, L}, shapeB[kChainGroups] = {L, Sh, Sh, L, L};
    const int nGroups = with_flush ? kChainGroups : kChainGroups - 1;
    const HostShape* hs[kChainGroups] = {};
    for (int g = 0; g < nGroups; ++g) {
        MRC_TRY(get_shape(h, shapeA[g], shapeB[g], &hs[g]));
        const DevShape& S = hs[g]->dev;
        if (const char* why = chain_shape_misfit(S, (g == 4 || !stereo) ? 1 : 2))
            return fail(h, MRC_ERR_INVALID, std::string("mrc_encode_chained: ") + why);
    }
    // ---- the schedule, pass 1: validate, sort the blocks into their shape groups (the offsets phase A needs).  The rest of
    // the schedule (items in file order, chunk maps, headers) is only needed by the serial scan and the packer: it is built
    // and uploaded in pass 2, AFTER phase A's launches are queued, so the device works while the host prepares it.
    const int64_t nItems = nB + (with_flush ? nch * n_streams : 0);
    const int64_t nChunks = nch * nB + (with_flush ? nch * n_streams : 0);
    std::vector<uint8_t> groupOf((size_t)nB);
    std::vector<int64_t> offs[kChainGroups];
    std::vector<long long> tailOff((size_t)n_streams);
    offs[0].reserve((size_t)nB);
    for (int64_t s = 0; s < n_streams; ++s) {
        const int64_t i0 = block_start[s], i1 = block_start[s + 1];
        if (i1 <= i0) return fail(h, MRC_ERR_INVALID, "mrc_encode_chained: every stream needs at least one block");
        for (int64_t i = i0; i < i1; ++i) {
            const int a = block_a[i], b = block_b[i];
            int g = -1;
            for (int q = 0; q < 4; ++q) if (a == shapeA[q] && b == shapeB[q]) { g = q; break; }   // (L == Sh: group 0)
            if (g < 0) return fail(h, MRC_ERR_INVALID, "mrc_encode_chained: block shape is not one of (L,L), (L,S), (S,S), (S,L)");
            const int64_t off = block_offset[i];
            if (off < 0 || off + a + b > stream_stride)
                return fail(h, MRC_ERR_INVALID, "mrc_encode_chained: block reaches outside its stream");
            if (offs[g].size() >= (size_t)1 << 28) return fail(h, MRC_ERR_INVALID, "mrc_encode_chained: too many blocks of one shape");
            groupOf[(size_t)(i - b0)] = (uint8_t)g;
            offs[g].push_back(s * stream_stride + off);
        }
        if (with_flush) {
            if (block_b[i1 - 1] != L)
                return fail(h, MRC_ERR_INVALID, "mrc_encode_chained: a stream must end with a long block (the reference's "
                                                "Close() assumes it, pacfileThem.py:973-984)");
            tailOff[(size_t)s] = block_offset[i1 - 1] + block_a[i1 - 1];
        }
    }

    MRC_HIP(h, hipSetDevice(h->device));
    hipStream_t st = pick_stream(h, stream);
    ChainBufs& C = h->chain;
    for (auto& e : C.evT) if (!e) MRC_HIP(h, hipEventCreate(&e));
    std::vector<long long> pos(item_byte_offset ? (size_t)(R * nChunks) + 1 : 0), streamPos((size_t)(R * n_streams));
    std::vector<int32_t> resOut((size_t)(R * n_streams));
    // (filled in pass 2; declared here: the guard below outlives every host buffer a queued copy may still read)
    std::vector<int32_t> items, chunkStream, resIn;
    std::vector<long long> itemStart, firstChunk, itemChunk, chunkMap[kChainGroups];
    std::vector<uint8_t> hdr;
    std::vector<ChainGroupDev> desc((size_t)R * kChainGroups);   // [rate][group]
    long long total = 0;
    int bad = 0;
    DrainGuard guard{{st}};
    MRC_HIP(h, hipEventRecord(C.evT[0], st));
    if (with_flush) {
        // the tail offsets ride in the offsets buffer of group 4 (its blocks are laid out explicitly, stride 2 L)
        MRC_TRY(upload(h, C.g[4].offsets, tailOff, st));
        MRC_HIP(h, C.flushPcm.reserve((size_t)n_streams * nch * 2 * L * sampleBytes));
        MRC_HIP(h, launch_chain_flush_gather(n_streams, L, pcm_left, pcm_right, sample_format, stream_stride,
                                             C.g[4].offsets.as<long long>(), C.flushPcm.p, st));
    }
    // ---- phase A + prep, per block shape
    int64_t count[kChainGroups] = {};
    for (int g = 0; g < nGroups; ++g) {
        const DevShape& S = hs[g]->dev;
        const int joint = (g == 4 || !stereo) ? 0 : 1, nsig = joint ? 4 : 1, nstream = joint ? 2 : 1;
        const int64_t m = g == 4 ? nch * n_streams : (int64_t)offs[g].size();
        count[g] = m;
        ChainGroupBufs& B = C.g[g];
        const int nTot = nstream * S.nBands, nEv = (int)chain_events_per_block(S, joint);
        if (m > 0) {
            if (g != 4) MRC_TRY(upload(h, B.offsets, offs[g], st));
            MRC_HIP(h, B.lines.reserve((size_t)m * nsig * S.halfN * sizeof(double)));
            MRC_HIP(h, B.oscale.reserve((size_t)m * nsig * sizeof(int32_t)));
            MRC_HIP(h, B.smr.reserve((size_t)m * nsig * S.nBands * sizeof(double)));
            MRC_HIP(h, B.peak.reserve((size_t)m * nsig * S.nBands * sizeof(double)));
            if (joint) MRC_HIP(h, B.ms.reserve((size_t)m * S.nBands * sizeof(int32_t)));
            MRC_HIP(h, B.ev.reserve((size_t)m * nEv * sizeof(unsigned)));
            MRC_HIP(h, B.pre.reserve((size_t)m * (nEv + 1) * sizeof(unsigned)));
            MRC_HIP(h, B.bitAlloc.reserve((size_t)R * m * nTot * sizeof(int32_t)));          // (phase B's planes: one per rate)
            MRC_HIP(h, B.scaleFactor.reserve((size_t)R * m * nTot * sizeof(int32_t)));
            MRC_HIP(h, B.mant.reserve((size_t)R * m * nstream * S.halfN * sizeof(uint16_t)));
            MRC_HIP(h, B.table.reserve((size_t)R * m * nstream * sizeof(int32_t)));
            if (g == 4)
                MRC_TRY(encode_phase_a(h, S, m, C.flushPcm.p, nullptr, sample_format, 2 * (int64_t)L, nullptr, B.lines.as<double>(),
                                       B.oscale.as<int32_t>(), nullptr, B.smr.as<double>(), B.peak.as<double>(), st, false));
            else                                             // (pcm_right == nullptr: the mono kernels, no M/S switch)
                MRC_TRY(encode_phase_a(h, S, m, pcm_left, pcm_right, sample_format, 0, B.offsets.as<int64_t>(),
                                       B.lines.as<double>(), B.oscale.as<int32_t>(), joint ? B.ms.as<int32_t>() : nullptr,
                                       B.smr.as<double>(), B.peak.as<double>(), st, false));
            MRC_HIP(h, launch_chain_prep(S, joint, m, B.smr.as<double>(), joint ? B.ms.as<int32_t>() : nullptr,
                                         B.ev.as<unsigned>(), B.pre.as<unsigned>(),
                                         h->chainForceFallback ? 1 : 0, st));
        }
        for (int r = 0; r < R; ++r) {
            // rate r: the shared phase-A data, its own budgets and output planes
            ChainGroupDev& D = desc[(size_t)r * kChainGroups + g];
            D = chain_group_desc(*hs[g], joint, B.lines.as<double>(), B.peak.as<double>(), B.oscale.as<int32_t>(),
                                 joint ? B.ms.as<int32_t>() : nullptr, B.ev.as<unsigned>(), B.pre.as<unsigned>(),
                                 B.bitAlloc.as<int32_t>() + r * m * nTot, B.scaleFactor.as<int32_t>() + r * m * nTot,
                                 B.mant.as<unsigned short>() + r * m * nstream * S.halfN, B.table.as<int32_t>() + r * m * nstream);
            if (rates) shape_budgets(cfg, rates[r], S.a, S.b, S.nBands, &D.budgetMono, &D.budgetJointPre);
        }
    }
    // ---- the schedule, pass 2 (the device is busy with phase A): items (group << 28 | index inside the group) per stream in
    // file order, the chunk of every item, the stream of every chunk, the chunks of every group
    items.resize((size_t)nItems);
    itemStart.resize((size_t)n_streams + 1); firstChunk.resize((size_t)n_streams);
    itemChunk.resize((size_t)nItems + 1);
    chunkStream.resize((size_t)(R * nChunks));
    resIn.assign((size_t)(R * n_streams), 0);
    for (int g = 0; g < 4; ++g) chunkMap[g].resize(R * nch * offs[g].size());
    if (with_flush) chunkMap[4].resize((size_t)(R * nch * n_streams));
    {
        int64_t it = 0, ch = 0;
        size_t idx[kChainGroups] = {};
        for (int64_t s = 0; s < n_streams; ++s) {
            itemStart[(size_t)s] = it;
            firstChunk[(size_t)s] = ch;
            for (int64_t i = block_start[s]; i < block_start[s + 1]; ++i) {
                const int g = groupOf[(size_t)(i - b0)];
                const size_t k = idx[g]++;
                items[(size_t)it] = (int32_t)((unsigned)g << 28 | (unsigned)k);
                itemChunk[(size_t)it] = ch;
                for (int c = 0; c < nch; ++c) {
                    chunkMap[g][nch * k + c] = ch;
                    chunkStream[(size_t)ch++] = (int32_t)s;
                }
                ++it;
            }
            if (with_flush)
                for (int c = 0; c < nch; ++c) {                    // codec.Encode: channel after channel
                    items[(size_t)it] = (int32_t)(4u << 28 | (unsigned)(nch * s + c));
                    chunkMap[4][(size_t)(nch * s + c)] = ch;
                    itemChunk[(size_t)it] = ch;
                    chunkStream[(size_t)ch] = (int32_t)s;
                    ++ch; ++it;
                }
        }
        itemStart[(size_t)n_streams] = it;
        itemChunk[(size_t)nItems] = ch;
        if (reservoir_in) for (int64_t q = 0; q < R * n_streams; ++q) resIn[(size_t)q] = reservoir_in[q];
        // rates after the first: their chunks behind all of the previous rate's, (rate, stream) the "stream" of each
        for (int r = 1; r < R; ++r) {
            for (int64_t c = 0; c < nChunks; ++c) chunkStream[(size_t)(r * nChunks + c)] = (int32_t)(r * n_streams) + chunkStream[(size_t)c];
            for (int g = 0; g < nGroups; ++g) {
                const size_t n1 = chunkMap[g].size() / R;           // (the group's chunks of one rate)
                for (size_t k = 0; k < n1; ++k) chunkMap[g][r * n1 + k] = r * nChunks + chunkMap[g][k];
            }
        }
        for (int r = 1; r < R; ++r)
            for (int64_t s = 0; s < n_streams; ++s) firstChunk.push_back(r * nChunks + firstChunk[(size_t)s]);
    }
    // ---- file headers (pacfileThem.py:586-613)
    int hdrLen = 0;
    if (num_samples) {
        // one header built by mrc_pac_header; the streams differ only in the sample count (bytes 10..13, little endian, with
        // the reference's padding rule, pacfileThem.py:595-597: padded when it ALREADY is a multiple of nMDCTLines)
        uint8_t one[256];
        int64_t len = 0;
        if (mrc_pac_header(&cfg, nch, num_samples[0], one, sizeof(one), &len) != MRC_OK || len < 14)
            return fail(h, MRC_ERR_INVALID, "mrc_encode_chained: mrc_pac_header failed");
        hdrLen = (int)len;
        hdr.resize((size_t)(R * n_streams) * len);                 // (the same headers in front of every rate's streams)
        for (int64_t s = 0; s < R * n_streams; ++s) {
            uint8_t* dst = hdr.data() + s * len;
            std::memcpy(dst, one, (size_t)len);
            uint32_t ns = num_samples[s % n_streams];
            if (ns % (uint32_t)cfg.n_mdct_lines == 0) ns += (uint32_t)cfg.n_mdct_lines;
            for (int q = 0; q < 4; ++q) dst[10 + q] = (uint8_t)(ns >> (8 * q));
        }
    }
    MRC_TRY(upload(h, C.items, items, st));
    MRC_TRY(upload(h, C.itemStart, itemStart, st));
    MRC_TRY(upload(h, C.reservoir, resIn, st));
    MRC_TRY(upload(h, C.chunkStream, chunkStream, st));
    MRC_TRY(upload(h, C.hdr, hdr, st));
    MRC_TRY(upload(h, C.firstChunk, firstChunk, st));
    for (int g = 0; g < nGroups; ++g)
        if (count[g] > 0) MRC_TRY(upload(h, C.g[g].chunkMap, chunkMap[g], st));
    if (reservoir_trace) MRC_HIP(h, C.resTrace.reserve((size_t)(R * nItems) * sizeof(int32_t)));
    MRC_TRY(upload(h, C.groupDesc, desc, st));
    MRC_HIP(h, hipEventRecord(C.evT[1], st));
    // ---- phase B: the serial scan per stream and rate
    MRC_HIP(h, launch_chain_phase_b(n_streams, R, C.groupDesc.as<ChainGroupDev>(), C.items.as<int>(), C.itemStart.as<long long>(),
                                    C.reservoir.as<int>(), reservoir_trace ? C.resTrace.as<int>() : nullptr, nItems,
                                    use_huffman ? 1 : 0, h->chainThreads, st));
    MRC_HIP(h, hipEventRecord(C.evT[2], st));
    if (h->sensOn)                                       // MRC_OPT_SENSITIVITY: the scan's decisions, group by group
        for (int g = 0; g < nGroups; ++g) {
            ChainGroupBufs& B = C.g[g];
            const int joint = desc[g].joint;                 // (one rate: the ladder refuses the option)
            MRC_HIP(h, launch_sensitivity(hs[g]->dev, count[g], joint, B.lines.as<double>(), B.oscale.as<int32_t>(),
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
    for (int g = 0; g < nGroups; ++g) {
        const int joint = desc[g].joint;
        P[g] = pack_params(cfg, shapeA[g], shapeB[g], joint ? 2 : 1, joint, use_huffman);
        if (!count[g]) continue;
        ChainGroupBufs& B = C.g[g];
        const int64_t nBlk = count[g];                              // (a mono item is a one-channel block)
        for (int r = 0; r < R; ++r) {
            const ChainGroupDev& D = desc[(size_t)r * kChainGroups + g];
            MRC_HIP(h, launch_pack_plan(hs[g]->dev, P[g], tables, nBlk, D.bitAlloc, D.mant, MRC_MANTISSA_I16, D.table, D.table,
                                        nullptr, W, B.chunkMap.as<long long>() + r * (chunkMap[g].size() / R),
                                        all_bands_non_empty(*hs[g]), st));
        }
    }
    MRC_HIP(h, launch_pack_scan(nChunksAll, 0, W, nullptr, num_samples ? C.chunkStream.as<int>() : nullptr, hdrLen, st));
    for (int g = 0; g < nGroups; ++g) {
        if (!count[g]) continue;
        ChainGroupBufs& B = C.g[g];
        const int bound = (int)(mrc_pack_bound(&cfg, shapeA[g], shapeB[g], 1, P[g].joint) - 4);
        for (int r = 0; r < R; ++r) {
            const ChainGroupDev& D = desc[(size_t)r * kChainGroups + g];
            MRC_HIP(h, launch_pack_write(hs[g]->dev, P[g], tables, count[g], B.oscale.as<int>(), P[g].joint ? B.ms.as<int>() : nullptr,
                                         D.scaleFactor, D.bitAlloc, D.mant, MRC_MANTISSA_I16, D.table, W,
                                         B.chunkMap.as<long long>() + r * (chunkMap[g].size() / R), out, (long long)out_cap, bound,
                                         all_bands_non_empty(*hs[g]), st));
        }
    }
    // the file headers (num_samples given), and the start of every (rate, stream)'s bytes
    MRC_HIP(h, C.streamPos.reserve((size_t)(R * n_streams) * sizeof(long long)));
    MRC_HIP(h, launch_chain_headers(R * n_streams, hdrLen, C.hdr.as<unsigned char>(), C.firstChunk.as<long long>(), W.pos, out,
                                    (long long)out_cap, C.streamPos.as<long long>(), st));
    MRC_HIP(h, hipEventRecord(C.evT[3], st));
    // ---- results: stream starts (the position of every chunk only if the caller asked for them), total, error flag,
    // reservoirs
    if (item_byte_offset)
        MRC_HIP(h, hipMemcpyAsync(pos.data(), W.pos, pos.size() * sizeof(long long), hipMemcpyDeviceToHost, st));
    MRC_HIP(h, hipMemcpyAsync(streamPos.data(), C.streamPos.p, streamPos.size() * sizeof(long long), hipMemcpyDeviceToHost, st));
    MRC_HIP(h, hipMemcpyAsync(&total, W.total, sizeof(total), hipMemcpyDeviceToHost, st));
    MRC_HIP(h, hipMemcpyAsync(&bad, W.errorFlag, sizeof(bad), hipMemcpyDeviceToHost, st));
    MRC_HIP(h, hipMemcpyAsync(resOut.data(), C.reservoir.p, resOut.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (reservoir_trace)
        MRC_HIP(h, hipMemcpyAsync(reservoir_trace, C.resTrace.p, (size_t)(R * nItems) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    MRC_HIP(h, hipStreamSynchronize(st));
    for (int i = 0; i < 3; ++i) {
        float ms = 0.f;
        MRC_HIP(h, hipEventElapsedTime(&ms, C.evT[i], C.evT[i + 1]));
        h->chainMs[i] = ms;
    }
    {
        float ms = 0.f;
        MRC_HIP(h, hipEventElapsedTime(&ms, C.evT[0], C.evT[3]));
        h->chainMs[3] = ms;
    }
    for (int r = 0; r < R; ++r) {
        // rate r's bytes: from its first stream's start to the next rate's (all rates' when one rate)
        const long long base = streamPos[(size_t)(r * n_streams)], end = r + 1 < R ? streamPos[(size_t)((r + 1) * n_streams)] : total;
        total_bytes[r] = end - base;
        if (rate_base) rate_base[r] = base;
        int64_t* so = stream_byte_offset + r * (n_streams + 1);
        for (int64_t s = 0; s < n_streams; ++s) so[s] = streamPos[(size_t)(r * n_streams + s)] - base;
        so[n_streams] = end - base;
        if (item_byte_offset) {
            int64_t* io = item_byte_offset + r * (nItems + 1);
            for (int64_t i = 0; i < nItems; ++i) io[i] = pos[(size_t)(r * nChunks + itemChunk[(size_t)i])] - base;
            io[nItems] = end - base;
        }
    }
    if (reservoir_out) std::memcpy(reservoir_out, resOut.data(), resOut.size() * sizeof(int32_t));
    if (bad & 3) return fail(h, MRC_ERR_INVALID, "mrc_encode_chained: internal error (table id / chunk size out of range)");
    if (total > out_cap || (bad & 4)) return fail(h, MRC_ERR_NOMEM, "mrc_encode_chained: out_cap too small (see total_bytes)");
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

// A chained encode cut into slabs, at n_rates bit rates (rates == nullptr: one, the handle's target_bits_per_sample).  The
// per-stream and per-item outputs hold one row per rate (see chained_core: [R][n_streams + 1], [R][n_items + 1], ...), with
// n_items the call's; out_cap[r] and total_bytes[r] per rate.
// sink(rate r, its slab bytes are at `buf` on the device, n of them, they belong at byte `at` of rate r's output) -> status
template <class Sink>
int chained_slabs(mrc_handle* h, int n_rates, const double* rates, int64_t n_streams, const void* pcm_left, const void* pcm_right,
                  int sample_format, int64_t stream_stride, const int64_t* block_start, const int64_t* block_offset,
                  const int32_t* block_a, const int32_t* block_b, const int32_t* reservoir_in, int use_huffman, int with_flush,
                  const uint32_t* num_samples, const int64_t* out_cap, int64_t* stream_byte_offset, int64_t* item_byte_offset,
                  int32_t* reservoir_out, int32_t* reservoir_trace, int64_t* total_bytes, void* stream,
                  uint8_t* direct_out /* one rate: device buffer of out_cap bytes to write into in place, or null: C.out per slab */,
                  Sink sink) {
    const int R = n_rates;
    if (!h || R < 1 || n_streams < 0 || !block_start || !stream_byte_offset || !total_bytes || !out_cap)
        return fail(h, MRC_ERR_INVALID, "mrc_encode_chained: bad argument");
    for (int r = 0; r < R; ++r) { total_bytes[r] = 0; stream_byte_offset[r * (n_streams + 1)] = 0; }
    if (n_streams == 0) return MRC_OK;
    for (int64_t s = 0; s < n_streams; ++s)
        if (block_start[s + 1] <= block_start[s]) return fail(h, MRC_ERR_INVALID, "mrc_encode_chained: every stream needs at least one block");
    const size_t sampleBytes = sample_format == MRC_SAMPLES_PCM16 ? sizeof(int16_t) : sizeof(double);
    const int nch = pcm_right ? 2 : 1;                   // (pcm_right == nullptr: mono streams)
    const int64_t nItemsAll = block_start[n_streams] - block_start[0] + (with_flush ? nch * n_streams : 0);
    const int64_t cap = h->chainSlabBlocks > 0 ? ladder_slab_blocks(h, h->chainSlabBlocks, R, nch) : (int64_t)1 << 40;
    const std::vector<Slab> slabs = plan_slabs(n_streams, block_start, cap);
    ChainBufs& C = h->chain;
    C.lastTotal = -1;
    int64_t itemBase = 0;
    std::vector<int64_t> written((size_t)R, 0), slabTotal((size_t)R), base((size_t)R);
    std::vector<char> overflow((size_t)R, 0);
    double ms[4] = {0, 0, 0, 0};
    std::vector<int64_t> sOff, iOff;
    std::vector<int32_t> carry((size_t)R, 0), resInSlab, resOutSlab, trace;
    for (const Slab& sl : slabs) {
        const char* pl = (const char*)pcm_left + (size_t)sl.s0 * stream_stride * sampleBytes;
        const char* pr = pcm_right ? (const char*)pcm_right + (size_t)sl.s0 * stream_stride * sampleBytes : nullptr;
        const int64_t bs2[2] = {sl.i0, sl.i1};
        const int64_t* bs = sl.timeSlab ? bs2 : block_start + sl.s0;
        const int flush = with_flush && sl.last;
        const uint32_t* nsamp = (num_samples && sl.first) ? num_samples + sl.s0 : nullptr;
        // the slab's reservoirs in: the previous time slab's, or the caller's rows of these streams
        const int32_t* resIn = nullptr;
        if (sl.timeSlab && !sl.first) resIn = carry.data();
        else if (reservoir_in) {
            resInSlab.resize((size_t)(R * sl.ns));
            for (int r = 0; r < R; ++r)
                for (int64_t s = 0; s < sl.ns; ++s) resInSlab[(size_t)(r * sl.ns + s)] = reservoir_in[r * n_streams + sl.s0 + s];
            resIn = resInSlab.data();
        }
        const int64_t nItems = (sl.i1 - sl.i0) + (flush ? nch * sl.ns : 0);
        sOff.assign((size_t)(R * (sl.ns + 1)), 0);
        if (item_byte_offset) iOff.assign((size_t)(R * (nItems + 1)), 0);
        resOutSlab.assign((size_t)(R * sl.ns), 0);
        if (reservoir_trace) trace.assign((size_t)(R * nItems), 0);
        uint8_t* dst;
        int64_t slabCap;
        if (direct_out && !overflow[0]) { dst = direct_out + written[0]; slabCap = out_cap[0] - written[0]; }
        else {
            const int64_t bound = mrc_chain_out_bound_ex(h, nch, sl.ns, bs, block_a, block_b, flush, nsamp != nullptr);
            if (bound < 0) return fail(h, MRC_ERR_INVALID, "mrc_encode_chained: block shape out of range");
            MRC_HIP(h, hipSetDevice(h->device));
            MRC_HIP(h, C.out.reserve((size_t)(R * bound) + 1));
            dst = C.out.as<uint8_t>(); slabCap = R * bound;
        }
        int rc = chained_core(h, R, rates, sl.ns, pl, pr, sample_format, stream_stride, bs, block_offset, block_a, block_b, resIn,
                              use_huffman, flush, nsamp, dst, slabCap, sOff.data(), item_byte_offset ? iOff.data() : nullptr,
                              resOutSlab.data(), reservoir_trace ? trace.data() : nullptr, slabTotal.data(), base.data(), stream);
        if (rc == MRC_ERR_NOMEM && direct_out) overflow[0] = 1;          // the caller's buffer is full: sizes only from here on
        else if (rc != MRC_OK) return rc;
        for (int i = 0; i < 4; ++i) ms[i] += h->chainMs[i];
        for (int r = 0; r < R; ++r) {
            int64_t* so = stream_byte_offset + r * (n_streams + 1);
            const int64_t* slabSo = sOff.data() + r * (sl.ns + 1);
            if (sl.timeSlab) {
                carry[(size_t)r] = resOutSlab[(size_t)r];
                if (sl.first) so[sl.s0] = written[(size_t)r] + slabSo[0];
                if (sl.last) {
                    so[sl.s0 + 1] = written[(size_t)r] + slabTotal[(size_t)r];
                    if (reservoir_out) reservoir_out[r * n_streams + sl.s0] = carry[(size_t)r];
                }
            } else {
                for (int64_t s = 0; s <= sl.ns; ++s) so[sl.s0 + s] = written[(size_t)r] + slabSo[s];
                if (reservoir_out)
                    for (int64_t s = 0; s < sl.ns; ++s) reservoir_out[r * n_streams + sl.s0 + s] = resOutSlab[(size_t)(r * sl.ns + s)];
            }
            if (item_byte_offset)
                for (int64_t i = 0; i <= nItems; ++i)
                    item_byte_offset[r * (nItemsAll + 1) + itemBase + i] = written[(size_t)r] + iOff[(size_t)(r * (nItems + 1) + i)];
            if (reservoir_trace && nItems)
                std::memcpy(reservoir_trace + r * nItemsAll + itemBase, trace.data() + r * nItems, (size_t)nItems * sizeof(int32_t));
            if (!direct_out && !overflow[(size_t)r]) {
                if (written[(size_t)r] + slabTotal[(size_t)r] > out_cap[r]) overflow[(size_t)r] = 1;
                else MRC_TRY(sink(r, dst + base[(size_t)r], slabTotal[(size_t)r], written[(size_t)r]));
            }
            written[(size_t)r] += slabTotal[(size_t)r];
        }
        itemBase += nItems;
    }
    for (int i = 0; i < 4; ++i) h->chainMs[i] = ms[i];
    bool full = false;
    for (int r = 0; r < R; ++r) {
        total_bytes[r] = written[(size_t)r];
        stream_byte_offset[r * (n_streams + 1) + n_streams] = written[(size_t)r];
        full = full || overflow[(size_t)r] || written[(size_t)r] > out_cap[r];
    }
    if (R == 1 && slabs.size() == 1 && !direct_out) C.lastTotal = written[0];   // (one slab: its bytes are all in C.out, mrc_chain_fetch_output)
    if (full) return fail(h, MRC_ERR_NOMEM, "mrc_encode_chained: out_cap too small (see total_bytes)");
    return MRC_OK;
}

// stage the host PCM of a host-memory entry point in the handle's device buffers
int stage_pcm(mrc_handle* h, int64_t n_streams, const void* pcm_left, const void* pcm_right, int sample_format,
              int64_t stream_stride) {
    ChainBufs& C = h->chain;
    const size_t pcmBytes = (size_t)n_streams * stream_stride * (sample_format == MRC_SAMPLES_PCM16 ? sizeof(int16_t) : sizeof(double));
    MRC_HIP(h, C.pcmL.reserve(pcmBytes ? pcmBytes : 1));
    if (pcm_right) MRC_HIP(h, C.pcmR.reserve(pcmBytes ? pcmBytes : 1));      // (mono streams: no right channel)
    DrainGuard guard{{h->stream}};
    if (pcmBytes) {
        MRC_HIP(h, hipMemcpyAsync(C.pcmL.p, pcm_left, pcmBytes, hipMemcpyHostToDevice, h->stream));
        if (pcm_right) MRC_HIP(h, hipMemcpyAsync(C.pcmR.p, pcm_right, pcmBytes, hipMemcpyHostToDevice, h->stream));
    }
    return MRC_OK;
}

// the ladder's own refusals (then every check of a one-rate call)
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

}  // namespace

extern "C" {

int mrc_dev_encode_chained_pac(mrc_handle* h, int64_t n_streams, const void* pcm_left, const void* pcm_right,
                               int sample_format, int64_t stream_stride, const int64_t* block_start, const int64_t* block_offset,
                               const int32_t* block_a, const int32_t* block_b, const int32_t* reservoir_in,
                               int use_huffman, int with_flush, const uint32_t* num_samples, uint8_t* out, int64_t out_cap,
                               int64_t* stream_byte_offset, int64_t* item_byte_offset, int32_t* reservoir_out,
                               int32_t* reservoir_trace, int64_t* total_bytes, void* stream) {
    if (!h || !pcm_left || stream_stride <= 0 || !block_offset || !block_a || !block_b || !out || out_cap < 0 ||
        (sample_format != MRC_SAMPLES_F64 && sample_format != MRC_SAMPLES_PCM16))
        return fail(h, MRC_ERR_INVALID, "mrc_encode_chained: bad argument");
    return chained_slabs(h, 1, nullptr, n_streams, pcm_left, pcm_right, sample_format, stream_stride, block_start, block_offset,
                         block_a, block_b, reservoir_in, use_huffman, with_flush, num_samples, &out_cap, stream_byte_offset,
                         item_byte_offset, reservoir_out, reservoir_trace, total_bytes, stream, out,
                         [](int, uint8_t*, int64_t, int64_t) { return (int)MRC_OK; });
}

int mrc_encode_chained_stream_pac(mrc_handle* h, int64_t n_streams, const void* pcm_left, const void* pcm_right,
                                  int sample_format, int64_t stream_stride, const int64_t* block_start,
                                  const int64_t* block_offset, const int32_t* block_a, const int32_t* block_b,
                                  const int32_t* reservoir_in, int use_huffman, int with_flush, const uint32_t* num_samples,
                                  uint8_t* out, int64_t out_cap, int64_t* stream_byte_offset, int64_t* item_byte_offset,
                                  int32_t* reservoir_out, int32_t* reservoir_trace, int64_t* total_bytes) {
    if (!h || n_streams < 0 || !pcm_left || stream_stride <= 0 || !out || !total_bytes || !block_start ||
        (sample_format != MRC_SAMPLES_F64 && sample_format != MRC_SAMPLES_PCM16))
        return fail(h, MRC_ERR_INVALID, "mrc_encode_chained_stream_pac: bad argument");
    MRC_HIP(h, hipSetDevice(h->device));
    MRC_TRY(stage_pcm(h, n_streams, pcm_left, pcm_right, sample_format, stream_stride));
    ChainBufs& C = h->chain;
    // every slab packs into the handle's device buffer (sized for the slab's worst case) and its bytes are copied behind the
    // previous slab's in the caller's buffer, which only has to hold what the streams really pack to
    hipStream_t st = h->stream;
    mrc_handle* hh = h;
    int rc = chained_slabs(h, 1, nullptr, n_streams, C.pcmL.p, pcm_right ? C.pcmR.p : nullptr, sample_format, stream_stride,
                           block_start, block_offset, block_a, block_b, reservoir_in, use_huffman, with_flush, num_samples, &out_cap,
                           stream_byte_offset, item_byte_offset, reservoir_out, reservoir_trace, total_bytes, h->stream, nullptr,
                           [out, st, hh](int, uint8_t* buf, int64_t n, int64_t at) {
                               if (n) MRC_HIP(hh, hipMemcpyAsync(out + at, buf, (size_t)n, hipMemcpyDeviceToHost, st));
                               MRC_HIP(hh, hipStreamSynchronize(st));      // (the next slab reuses the buffer)
                               return (int)MRC_OK;
                           });
    if (rc == MRC_ERR_NOMEM)
        return fail(h, MRC_ERR_NOMEM, "mrc_encode_chained_stream_pac: out_cap too small (see total_bytes; mrc_chain_fetch_output)");
    return rc;
}

int mrc_encode_chained_ladder_pac(mrc_handle* h, int n_rates, const double* target_bits_per_sample, int64_t n_streams,
                                  const void* pcm_left, const void* pcm_right, int sample_format, int64_t stream_stride,
                                  const int64_t* block_start, const int64_t* block_offset, const int32_t* block_a,
                                  const int32_t* block_b, const int32_t* reservoir_in, int use_huffman, int with_flush,
                                  const uint32_t* num_samples, uint8_t* const* out, const int64_t* out_cap,
                                  int64_t* stream_byte_offset, int64_t* item_byte_offset, int32_t* reservoir_out,
                                  int32_t* reservoir_trace, int64_t* total_bytes) {
    MRC_TRY(ladder_check(h, "mrc_encode_chained_ladder_pac", n_rates, target_bits_per_sample, out, out_cap, total_bytes));
    if (n_streams < 0 || !pcm_left || stream_stride <= 0 || !block_start || !block_offset || !block_a || !block_b ||
        (sample_format != MRC_SAMPLES_F64 && sample_format != MRC_SAMPLES_PCM16))
        return fail(h, MRC_ERR_INVALID, "mrc_encode_chained_ladder_pac: bad argument");
    h->chain.lastTotal = -1;                             // (whatever happens: no output of a one-rate call is served after this)
    MRC_HIP(h, hipSetDevice(h->device));
    MRC_TRY(stage_pcm(h, n_streams, pcm_left, pcm_right, sample_format, stream_stride));
    ChainBufs& C = h->chain;
    hipStream_t st = h->stream;
    mrc_handle* hh = h;
    int rc = chained_slabs(h, n_rates, target_bits_per_sample, n_streams, C.pcmL.p, pcm_right ? C.pcmR.p : nullptr, sample_format,
                           stream_stride, block_start, block_offset, block_a, block_b, reservoir_in, use_huffman, with_flush,
                           num_samples, out_cap, stream_byte_offset, item_byte_offset, reservoir_out, reservoir_trace, total_bytes,
                           h->stream, nullptr,
                           [out, st, hh](int r, uint8_t* buf, int64_t n, int64_t at) {
                               if (n) MRC_HIP(hh, hipMemcpyAsync(out[r] + at, buf, (size_t)n, hipMemcpyDeviceToHost, st));
                               MRC_HIP(hh, hipStreamSynchronize(st));      // (the next slab reuses the buffer)
                               return (int)MRC_OK;
                           });
    if (rc == MRC_ERR_NOMEM)
        return fail(h, MRC_ERR_NOMEM, "mrc_encode_chained_ladder_pac: an out_cap too small (see total_bytes)");
    return rc;
}

int mrc_dev_encode_chained_ladder_pac(mrc_handle* h, int n_rates, const double* target_bits_per_sample, int64_t n_streams,
                                      const void* pcm_left, const void* pcm_right, int sample_format, int64_t stream_stride,
                                      const int64_t* block_start, const int64_t* block_offset, const int32_t* block_a,
                                      const int32_t* block_b, const int32_t* reservoir_in, int use_huffman, int with_flush,
                                      const uint32_t* num_samples, uint8_t* const* out, const int64_t* out_cap,
                                      int64_t* stream_byte_offset, int64_t* item_byte_offset, int32_t* reservoir_out,
                                      int32_t* reservoir_trace, int64_t* total_bytes, void* stream) {
    MRC_TRY(ladder_check(h, "mrc_dev_encode_chained_ladder_pac", n_rates, target_bits_per_sample, out, out_cap, total_bytes));
    if (n_streams < 0 || !pcm_left || stream_stride <= 0 || !block_start || !block_offset || !block_a || !block_b ||
        (sample_format != MRC_SAMPLES_F64 && sample_format != MRC_SAMPLES_PCM16))
        return fail(h, MRC_ERR_INVALID, "mrc_dev_encode_chained_ladder_pac: bad argument");
    h->chain.lastTotal = -1;
    MRC_HIP(h, hipSetDevice(h->device));
    hipStream_t st = pick_stream(h, stream);
    mrc_handle* hh = h;
    // each slab's bytes of rate r: device to device behind the previous slab's in out[r] (ordered on `st` before the next
    // slab packs into the same buffer)
    int rc = chained_slabs(h, n_rates, target_bits_per_sample, n_streams, pcm_left, pcm_right, sample_format, stream_stride,
                           block_start, block_offset, block_a, block_b, reservoir_in, use_huffman, with_flush, num_samples, out_cap,
                           stream_byte_offset, item_byte_offset, reservoir_out, reservoir_trace, total_bytes, st, nullptr,
                           [out, st, hh](int r, uint8_t* buf, int64_t n, int64_t at) {
                               if (n) MRC_HIP(hh, hipMemcpyAsync(out[r] + at, buf, (size_t)n, hipMemcpyDeviceToDevice, st));
                               return (int)MRC_OK;
                           });
    if (rc == MRC_OK || rc == MRC_ERR_NOMEM) MRC_HIP(h, hipStreamSynchronize(st));
    if (rc == MRC_ERR_NOMEM)
        return fail(h, MRC_ERR_NOMEM, "mrc_dev_encode_chained_ladder_pac: an out_cap too small (see total_bytes)");
    return rc;
}

int mrc_chain_fetch_output(mrc_handle* h, uint8_t* out, int64_t out_cap, int64_t* total_bytes) {
    if (!h || !out || !total_bytes) return fail(h, MRC_ERR_INVALID, "mrc_chain_fetch_output: bad argument");
    ChainBufs& C = h->chain;
    if (C.lastTotal < 0) return fail(h, MRC_ERR_INVALID, "mrc_chain_fetch_output: no output of a chained call is held");
    *total_bytes = C.lastTotal;
    if (C.lastTotal > out_cap) return fail(h, MRC_ERR_NOMEM, "mrc_chain_fetch_output: out_cap too small (see total_bytes)");
    MRC_HIP(h, hipSetDevice(h->device));
    if (C.lastTotal) MRC_HIP(h, hipMemcpyAsync(out, C.out.p, (size_t)C.lastTotal, hipMemcpyDeviceToHost, h->stream));
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
