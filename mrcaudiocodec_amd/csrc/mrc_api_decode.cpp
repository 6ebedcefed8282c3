// Decode of whole `.pac` files on the device: the host reads headers, chunk lengths and each chunk's block-switch bits
// (4 bits into its payload) -- enough to know every block's shape and where its samples go -- and nothing else.  Bytes and
// plan cross PCIe in one copy; chunk parsing (unpack_dense_kernel), dequantisation / IMDCT / overlap-add
// (decode_kernel, unchanged) and the interleaved 16-bit codes (pcm16_interleave_kernel) run on the device; one copy
// brings the WAV-order samples back.
//
// Blocks are grouped exactly as pacfile.decode_pac groups them: a stereo file of more than one block is joint blocks
// followed by the two non-joint chunks Close() wrote (pacfileThem.py:973-984), every other file is non-joint blocks.
// A group is a (block shape, kind): one decode_kernel launch each, over all files of the call.  The output planes hold
// every file one after the other, channel 1 one plane stride behind channel 0; each output sample receives at most two
// atomic contributions, so the order of the blocks does not change a bit of the result.
//
// Also here, for mrc_api_nmr.cpp and mrc_api_store.cpp as well: the host plan (pac_plan_scan / pac_plan_groups /
// pac_plan_layout), the preamble of a call that takes a list of files (check_file_list) and the parse step (pac_parse: staging
// copy, unpack_dense_kernel, verdict, a bad chunk named by file and byte).  Their pure parts -- the staging layout, the chunk
// locator, the slots a block takes -- are in mrc_pac_stage.hpp; the walk over the groups that have slots (decode_groups) is in
// mrc_handle.hpp.
#include "mrc_handle.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <thread>

using namespace mrc;

namespace mrc {

UnpackParams unpack_params(const mrc_config& c) {
    UnpackParams P;
    P.nScaleBits = c.n_scale_bits;
    P.nMantSizeBits = c.n_mant_size_bits;
    P.blkBitsA = c.blksw_bits_a;
    P.blkBitsB = c.blksw_bits_b;
    P.nShort = c.n_short;
    P.nLines = c.n_mdct_lines;
    return P;
}

// the band counts of the four shapes as the parser sees them (-1: a shape without a usable band table); host only
void decode_band_counts(const mrc_config& c, int nBands[4], std::vector<int>* cnt /* nullable: [4] */) {
    for (int s = 0; s < 4; ++s) {
        int a, b;
        shape_ab(c, s, &a, &b);
        std::vector<int> tmp;
        std::vector<int>& v = cnt ? cnt[s] : tmp;
        // (a shape of more lines than n_mdct_lines would not fit mrc_unpack_blocks' fixed stride either: refused)
        if (!band_table(c, a, b, &v) || (int)v.size() > MRC_MAX_BANDS || (a + b) / 2 > c.n_mdct_lines)
            v.clear(), nBands[s] = -1;
        else nBands[s] = (int)v.size();
    }
}

// decode tables + band tables of the four shapes in device memory, once per handle
int ensure_decode_consts(mrc_handle* h) {
    DecodeBufs& d = h->dec;
    MRC_HIP(h, hipSetDevice(h->device));
    if (d.consts.p) return MRC_OK;
    std::vector<int> cnt[4];
    StageLayout lay(256);                                // UnpackTables | the four band tables
    size_t bandOff[4];
    lay.add<UnpackTables>(1);
    decode_band_counts(h->cfg, d.bands.nBands, cnt);
    for (int s = 0; s < 4; ++s) {
        int a, b;
        shape_ab(h->cfg, s, &a, &b);
        d.bands.halfN[s] = (a + b) / 2;
        bandOff[s] = lay.add<int>(cnt[s].size() + 1);
    }
    const size_t bytes = lay.total();
    std::vector<unsigned char> blob(bytes, 0);
    unpack_tables((UnpackTables*)blob.data());
    for (int s = 0; s < 4; ++s)
        if (!cnt[s].empty()) std::memcpy(blob.data() + bandOff[s], cnt[s].data(), sizeof(int) * cnt[s].size());
    MRC_HIP(h, d.consts.reserve(bytes));
    MRC_HIP(h, hipMemcpy(d.consts.p, blob.data(), bytes, hipMemcpyHostToDevice));
    for (int s = 0; s < 4; ++s) d.bands.bandN[s] = (const int*)(d.consts.as<unsigned char>() + bandOff[s]);
    if (!d.pinErr) MRC_HIP(h, pinned_alloc(&d.pinErr, sizeof(UnpackErr)));
    MRC_HIP(h, d.ev.create());
    return MRC_OK;
}

const char* unpack_status_text(int flag) {
    if (flag & (1 << kUnpackBadTable)) return "table id not in {0..3, 15}";
    if (flag & (1 << kUnpackBadAlloc)) return "bit allocation above 16";
    if (flag & (1 << kUnpackBadCode)) return "bits that are no Huffman code of the table";
    if (flag & (1 << kUnpackBadShape)) return "block shape without a band table or not the block's";
    return "read past the end of a chunk";
}

// err <- {0, INT_MAX} on the stream
int reset_unpack_err(mrc_handle* h, hipStream_t st) {
    DecodeBufs& d = h->dec;
    MRC_HIP(h, d.err.reserve(sizeof(UnpackErr)));
    UnpackErr* e = d.err.as<UnpackErr>();
    MRC_HIP(h, hipMemsetAsync(&e->flag, 0, sizeof(int), st));
    MRC_HIP(h, hipMemsetD32Async((hipDeviceptr_t)&e->firstBad, 0x7fffffff, 1, st));
    return MRC_OK;
}

int read_unpack_err(mrc_handle* h, hipStream_t st, const UnpackErr** bad) {
    DecodeBufs& d = h->dec;
    MRC_HIP(h, hipMemcpyAsync(d.pinErr.get(), d.err.p, sizeof(UnpackErr), hipMemcpyDeviceToHost, st));
    MRC_HIP(h, hipStreamSynchronize(st));
    *bad = d.pinErr->flag ? d.pinErr.get() : nullptr;
    return MRC_OK;
}

int pac_parse(mrc_handle* h, const char* fn, const std::vector<int64_t>& fileBase, const PacParse& p) {
    DecodeBufs& d = h->dec;
    const unsigned char* dev = (const unsigned char*)p.dev;
    MRC_HIP(h, hipEventRecord(p.ev[0], p.st));
    MRC_HIP(h, hipMemcpyAsync(p.dev, p.pin, p.total, hipMemcpyHostToDevice, p.st));
    MRC_HIP(h, hipEventRecord(p.ev[1], p.st));
    MRC_TRY(reset_unpack_err(h, p.st));
    MRC_HIP(h, launch_unpack_dense(unpack_params(h->cfg), d.bands, d.consts.as<UnpackTables>(), p.nChunks,
                                   (const UnpackPlanEntry*)(dev + p.oPlan), p.bytes, p.nBytes,
                                   (const UnpackGroupDev*)(dev + p.oGroups), d.err.as<UnpackErr>(), p.st));
    MRC_HIP(h, hipEventRecord(p.ev[2], p.st));
    const UnpackErr* bad;
    MRC_TRY(read_unpack_err(h, p.st, &bad));
    if (!bad) return MRC_OK;
    // (firstBad is the minimum over the flagged chunks, so it names one; were it not to, the answer is file 0, byte 0)
    const UnpackPlanEntry* plan = (const UnpackPlanEntry*)((const unsigned char*)p.pin + p.oPlan);
    const ChunkPlace at = bad->firstBad < p.nChunks ? pac_locate_chunk(fileBase, plan[bad->firstBad].off) : ChunkPlace{0, 0};
    char msg[240];
    std::snprintf(msg, sizeof msg, "%s: file %lld: chunk at byte %lld: %s", fn, (long long)at.file, (long long)at.byte,
                  unpack_status_text(bad->flag));
    return fail(h, MRC_ERR_INVALID, msg);
}

int check_file_list(mrc_handle* h, const char* fn, int64_t n_files, const uint8_t* buf, const int64_t* file_offset) {
    if (n_files < 0 || !file_offset || (n_files > 0 && !buf)) return fail(h, MRC_ERR_INVALID, std::string(fn) + ": bad argument");
    for (int64_t f = 0; f < n_files; ++f)
        if (file_offset[0] < 0 || file_offset[f + 1] < file_offset[f])
            return fail(h, MRC_ERR_INVALID, std::string(fn) + ": file_offset must not decrease");
    return MRC_OK;
}

// memcpy over a few host threads for large copies (page-locked staging <-> the caller's memory)
void copy_host(void* dst, const void* src, size_t n) {
    const size_t kSlice = (size_t)8 << 20;
    int nt = (int)std::min<size_t>(8, n / kSlice);
    if (nt <= 1) { std::memcpy(dst, src, n); return; }
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; ++t) {
        const size_t lo = n * t / nt, hi = n * (t + 1) / nt;
        pool.emplace_back([=] { std::memcpy((char*)dst + lo, (const char*)src + lo, hi - lo); });
    }
    for (auto& th : pool) th.join();
}

// ---- host plan, pass 1: headers, chunks, block shapes, where each file's samples go
// ONE file: header, the caller's parameters against the file's (`owner` words who named them), chunk scan with shape
// bits, block positions.  Appends the file's chunks (offsets + base) and fills fi except xStart.  h == nullptr: the
// text goes to mrc_last_error(NULL).
int pac_scan_file(mrc_handle* h, const mrc_config& hc, const char* fn, const char* owner, int64_t f, const uint8_t* fb,
                  int64_t flen, int64_t base, std::vector<int64_t>* chunkOff, std::vector<unsigned char>* chunkShape,
                  PacFilePlan* out) {
    const UnpackParams P = unpack_params(hc);
    int nBands[4];
    decode_band_counts(hc, nBands, nullptr);
    char msg[200];
    mrc_config fc = hc;
    int32_t nch = 0;
    uint32_t ns = 0;
    int64_t doff = 0;
    if (mrc_pac_read_header(fb, flen, &fc, &nch, &ns, &doff) != MRC_OK) {
        std::snprintf(msg, sizeof msg, "%s: file %lld: not a .pac header (", fn, (long long)f);
        return fail(h, MRC_ERR_INVALID, msg + create_error() + ")");
    }
    const struct { const char* name; int file, handle; } par[4] = {
        {"sample_rate", fc.sample_rate, hc.sample_rate}, {"n_mdct_lines", fc.n_mdct_lines, hc.n_mdct_lines},
        {"n_scale_bits", fc.n_scale_bits, hc.n_scale_bits}, {"n_mant_size_bits", fc.n_mant_size_bits, hc.n_mant_size_bits}};
    for (const auto& q : par)
        if (q.file != q.handle) {
            std::snprintf(msg, sizeof msg, "%s: file %lld has %s = %d, %s %d", fn, (long long)f, q.name, q.file, owner,
                          q.handle);
            return fail(h, MRC_ERR_INVALID, msg);
        }
    PacFilePlan& fi = *out;
    fi.nch = nch;
    fi.firstChunk = (int64_t)chunkOff->size();
    for (int64_t off = doff; off + 4 <= flen;) {       // mrc_pac_scan_chunks
        const int64_t nBytes = unpack_u32le(fb + off);
        if (off + 4 + nBytes > flen) {
            std::snprintf(msg, sizeof msg, "%s: file %lld: truncated chunk at byte %lld", fn, (long long)f,
                          (long long)off);
            return fail(h, MRC_ERR_INVALID, msg);
        }
        int shape;
        if (unpack_chunk_shape(fb + off + 4, nBytes, P, &shape) != kUnpackOk || nBands[shape] < 0) {
            std::snprintf(msg, sizeof msg, "%s: file %lld: chunk at byte %lld has no block shape", fn, (long long)f,
                          (long long)off);
            return fail(h, MRC_ERR_INVALID, msg);
        }
        chunkOff->push_back(base + off);
        chunkShape->push_back((unsigned char)shape);
        off += 4 + nBytes;
    }
    fi.nChunks = (int64_t)chunkOff->size() - fi.firstChunk;
    if (fi.nChunks % nch) {
        std::snprintf(msg, sizeof msg, "%s: file %lld: %lld chunks for %d channels", fn, (long long)f,
                      (long long)fi.nChunks, nch);
        return fail(h, MRC_ERR_INVALID, msg);
    }
    int64_t start = 0;
    for (int64_t i = 0; i < fi.nChunks / nch; ++i) {
        const int s = (*chunkShape)[(size_t)(fi.firstChunk + i * nch)];
        if (nch == 2 && (*chunkShape)[(size_t)(fi.firstChunk + i * nch + 1)] != s) {
            std::snprintf(msg, sizeof msg, "%s: file %lld: the chunks of block %lld differ in shape", fn, (long long)f,
                          (long long)i);
            return fail(h, MRC_ERR_INVALID, msg);
        }
        int a, b;
        shape_ab(hc, s, &a, &b);
        fi.extent = std::max(fi.extent, start + a + b);   // (a file whose shapes do not chain still stays in its plane)
        fi.total = start + a + b;                          // pacfile.decode_pac: last block's start + a + b
        start += a;
    }
    return MRC_OK;
}

int pac_plan_scan(mrc_handle* h, const char* fn, int64_t n_files, const uint8_t* buf, const int64_t* file_offset,
                  PacPlan* p) {
    p->files.assign((size_t)n_files, PacFilePlan{});
    p->fileBase = pac_file_bases(file_offset, n_files);
    p->chunkOff.clear();
    p->chunkShape.clear();
    p->planeStride = 0;
    p->anyStereo = false;
    for (int64_t f = 0; f < n_files; ++f) {
        PacFilePlan& fi = p->files[(size_t)f];
        MRC_TRY(pac_scan_file(h, h->cfg, fn, "the handle was created with", f, buf + file_offset[f],
                              file_offset[f + 1] - file_offset[f], p->fileBase[(size_t)f], &p->chunkOff,
                              &p->chunkShape, &fi));
        fi.xStart = p->planeStride;
        p->planeStride += fi.extent;
        p->anyStereo |= fi.nch == 2;
    }
    return MRC_OK;
}

// ---- pass 2: groups and slots
int pac_plan_groups(mrc_handle* h, const char* fn, PacPlan* p) {
    p->clear_counts();
    for (int64_t f = 0; f < (int64_t)p->files.size(); ++f)
        for (int64_t i = 0; i < p->nBlocks(f); ++i) p->add_block(p->shape(f, i), i < p->nJoint(f), p->files[(size_t)f].nch);
    return pac_plan_layout(h, fn, p);
}

// ... the part that follows from nSlots alone (mrc_pac_store_decode_window counts the slots of its windows itself)
int pac_plan_layout(mrc_handle* h, const char* fn, PacPlan* p) {
    const DecodeBufs& d = h->dec;
    for (int64_t g = 0, q = 0; g < kUnpackGroups; q += p->nSlots[g], ++g) p->slotBase[g] = q;
    for (int s = 0; s < 4; ++s) p->hs[s] = nullptr;
    for (int s = 0; s < 4; ++s)
        if (p->nSlots[s * 2] + p->nSlots[s * 2 + 1]) {
            int a, b;
            shape_ab(h->cfg, s, &a, &b);
            MRC_TRY(get_shape(h, a, b, &p->hs[s]));
            if (p->hs[s]->dev.nBands != d.bands.nBands[s])
                return fail(h, MRC_ERR_INVALID, std::string(fn) + ": band tables disagree");
        }
    StageLayout lay(256);
    for (int g = 0; g < kUnpackGroups; ++g) {
        const int s = g / 2, joint = !(g & 1), nb = std::max(d.bands.nBands[s], 0), half = d.bands.halfN[s];
        const int64_t n = p->nSlots[g], ns = joint ? 2 : 1;
        const size_t sz[5] = {sizeof(int) * n * (joint ? 4 : 1), joint ? sizeof(int) * n * nb : 0, sizeof(int) * n * ns * nb,
                              sizeof(int) * n * ns * nb, sizeof(int) * n * ns * half};
        for (int k = 0; k < 5; ++k) p->gOff[g][k] = lay.add(sz[k]);
    }
    p->gBytes = lay.total();
    return MRC_OK;
}

}  // namespace mrc

extern "C" {

int mrc_dev_unpack_blocks(mrc_handle* h, int64_t n_blocks, int n_channels, int joint, const uint8_t* buf, int64_t len,
                          const int64_t* chunk_offset, int32_t* a, int32_t* b, int32_t* huff_table, int32_t* overall_scale,
                          int32_t* ms_switch, int32_t* scale_factor, int32_t* bit_alloc, int32_t* mantissa, void* stream) {
    if (!h) return MRC_ERR_INVALID;
    const mrc_config& c = h->cfg;
    if (!buf || !chunk_offset || !a || !b || !huff_table || !overall_scale || !scale_factor || !bit_alloc || !mantissa ||
        n_blocks < 0 || n_channels < 1 || n_channels > 2 || (joint && (n_channels != 2 || !ms_switch)) || len < 0 ||
        c.n_mdct_lines <= 0 || c.n_scale_bits < 1 || c.n_scale_bits > 4 || c.n_mant_size_bits < 1 || c.n_mant_size_bits > 8)
        return fail(h, MRC_ERR_INVALID, "mrc_dev_unpack_blocks: bad argument");
    MRC_TRY(ensure_decode_consts(h));
    hipStream_t st = pick_stream(h, stream);
    MRC_TRY(reset_unpack_err(h, st));
    UnpackFixedOut O{a, b, huff_table, overall_scale, ms_switch, scale_factor, bit_alloc, mantissa};
    MRC_HIP(h, launch_unpack_fixed(unpack_params(c), h->dec.bands, h->dec.consts.as<UnpackTables>(), n_blocks, n_channels,
                                   joint ? 1 : 0, buf, len, chunk_offset, O, h->dec.err.as<UnpackErr>(), st));
    const UnpackErr* bad;
    MRC_TRY(read_unpack_err(h, st, &bad));
    if (bad) {
        char msg[160];
        std::snprintf(msg, sizeof msg, "mrc_dev_unpack_blocks: chunk %d: %s", bad->firstBad, unpack_status_text(bad->flag));
        return fail(h, MRC_ERR_INVALID, msg);
    }
    return MRC_OK;
}

int mrc_decode_pac_pcm16(mrc_handle* h, int64_t n_files, const uint8_t* buf, const int64_t* file_offset, int16_t* out,
                         int64_t out_cap, int64_t* sample_offset, int32_t* n_channels) {
    if (!h) return MRC_ERR_INVALID;
    const char* const fn = "mrc_decode_pac_pcm16";
    if (!sample_offset || !n_channels || out_cap < 0) return fail(h, MRC_ERR_INVALID, "mrc_decode_pac_pcm16: bad argument");
    MRC_TRY(check_file_list(h, fn, n_files, buf, file_offset));
    const int L = h->cfg.n_mdct_lines;
    char msg[200];
    sample_offset[0] = 0;
    if (n_files == 0) return MRC_OK;
    MRC_TRY(ensure_decode_consts(h));
    DecodeBufs& d = h->dec;

    // ---- host plan (shared with mrc_pac_nmr): headers, chunks, block shapes, where each file's samples go
    const int64_t inBytes = file_offset[n_files] - file_offset[0];
    PacPlan pl;
    MRC_TRY(pac_plan_scan(h, fn, n_files, buf, file_offset, &pl));
    const int64_t planeStride = pl.planeStride;
    for (int64_t f = 0; f < n_files; ++f) {
        const PacFilePlan& fi = pl.files[(size_t)f];
        n_channels[f] = fi.nch;
        sample_offset[f + 1] = sample_offset[f] + std::max<int64_t>(0, fi.total - L) * fi.nch;
    }
    const int64_t nOut = sample_offset[n_files];
    if (nOut > out_cap || (nOut > 0 && !out)) {
        std::snprintf(msg, sizeof msg, "mrc_decode_pac_pcm16: the files decode to %lld values, out_cap is %lld",
                      (long long)nOut, (long long)out_cap);
        return fail(h, MRC_ERR_NOMEM, msg);
    }

    // ---- pass 2: groups and slots; plan entries ordered by (group, joint channel) so that a wave parses one kind
    MRC_TRY(pac_plan_groups(h, fn, &pl));

    // staging layout (one H2D copy): bytes | plan | groups | block offsets | outStart [n+1] | xStart [n] | nch [n]
    StageLayout lay(256);
    const size_t oBytes = lay.add((size_t)inBytes), oPlan = lay.add<UnpackPlanEntry>(pl.nChunks()),
                 oGroups = lay.add<UnpackGroupDev>(kUnpackGroups), oOffs = lay.add<long long>(pl.totalSlots),
                 oOutStart = lay.add<long long>(n_files + 1), oXStart = lay.add<long long>(n_files),
                 oNch = lay.add<int>(n_files), inTotal = lay.total();
    const int64_t xDoubles = planeStride * (pl.anyStereo ? 2 : 1);
    MRC_HIP(h, d.pinIn.reserve(inTotal));
    MRC_HIP(h, d.in.reserve(inTotal));
    MRC_HIP(h, d.groups.reserve(std::max<size_t>(pl.gBytes, 256)));
    MRC_HIP(h, d.x.reserve(std::max<size_t>(sizeof(double) * xDoubles, 256)));
    MRC_HIP(h, d.pcm.reserve(std::max<size_t>(sizeof(int16_t) * nOut, 256)));
    MRC_HIP(h, d.pinOut.reserve(std::max<size_t>(sizeof(int16_t) * nOut, 256)));

    unsigned char* pin = (unsigned char*)d.pinIn.p;
    copy_host(pin + oBytes, buf + file_offset[0], (size_t)inBytes);
    UnpackGroupDev* gd = (UnpackGroupDev*)(pin + oGroups);
    long long* offs = (long long*)(pin + oOffs);
    long long* outStart = (long long*)(pin + oOutStart);
    long long* xStart = (long long*)(pin + oXStart);
    int* nchDev = (int*)(pin + oNch);
    pac_plan_fill(h->cfg, d, pl, (UnpackPlanEntry*)(pin + oPlan), gd, d.groups.as<unsigned char>(),
                  [&](int64_t f, int64_t, int g, int slot, int ch, int64_t start) {
                      offs[pl.slotBase[g] + slot] = ch * planeStride + pl.files[(size_t)f].xStart + start;
                  });
    for (int64_t f = 0; f < n_files; ++f) {
        outStart[f] = sample_offset[f];
        xStart[f] = pl.files[(size_t)f].xStart;
        nchDev[f] = pl.files[(size_t)f].nch;
    }
    outStart[n_files] = nOut;

    // ---- device: the parse step (the plan entries point into the staging's own bytes), synthesis, interleave
    hipStream_t st = h->stream;
    unsigned char* din = d.in.as<unsigned char>();
    MRC_TRY(pac_parse(h, fn, pl.fileBase, PacParse{pin, din, inTotal, oPlan, oGroups, pl.nChunks(), din + oBytes, inBytes,
                                                   {d.ev[0], d.ev[1], d.ev[2]}, st}));
    double* x = d.x.as<double>();
    MRC_HIP(h, hipMemsetAsync(x, 0, sizeof(double) * xDoubles, st));
    MRC_TRY(decode_groups(h, pl, gd, (const int64_t*)(din + oOffs), x, planeStride, st));
    short* pcm = d.pcm.as<short>();
    MRC_HIP(h, launch_pcm16_interleave(n_files, nOut, (const long long*)(din + oOutStart), (const long long*)(din + oXStart),
                                       (const int*)(din + oNch), L, x, planeStride, pcm, st));
    MRC_HIP(h, hipEventRecord(d.ev[3], st));
    if (nOut) MRC_HIP(h, hipMemcpyAsync(d.pinOut.p, pcm, sizeof(int16_t) * nOut, hipMemcpyDeviceToHost, st));
    MRC_HIP(h, hipEventRecord(d.ev[4], st));
    MRC_HIP(h, hipStreamSynchronize(st));
    for (int i = 0; i < 4; ++i) MRC_HIP(h, d.ev.elapsed(i, i + 1, &d.ms[i]));
    if (nOut) copy_host(out, d.pinOut.p, sizeof(int16_t) * nOut);
    return MRC_OK;
}

int mrc_pac_index(const mrc_config* cfg, const uint8_t* buf, int64_t len, int32_t* n_channels, int64_t* n_blocks,
                  int64_t* n_samples, int64_t block_cap, int64_t* block_start, int32_t* block_a, int32_t* block_b,
                  int64_t* chunk_offset) {
    if (!cfg || !buf || len < 0 || !n_channels || !n_blocks || !n_samples || block_cap < 0)
        return fail(nullptr, MRC_ERR_INVALID, "mrc_pac_index: bad argument");
    std::vector<int64_t> chunkOff;
    std::vector<unsigned char> chunkShape;
    PacFilePlan fi;
    MRC_TRY(pac_scan_file(nullptr, *cfg, "mrc_pac_index", "cfg has", 0, buf, len, 0, &chunkOff, &chunkShape, &fi));
    const int64_t nb = fi.nChunks / fi.nch;
    *n_channels = fi.nch;
    *n_blocks = nb;
    *n_samples = std::max<int64_t>(0, fi.total - cfg->n_mdct_lines);
    if (nb > block_cap || (nb > 0 && (!block_start || !block_a || !block_b || !chunk_offset)))
        return fail(nullptr, MRC_ERR_NOMEM, "mrc_pac_index: the file has " + std::to_string(nb) + " blocks, block_cap is " +
                                                std::to_string(block_cap));
    int64_t start = 0;
    for (int64_t i = 0; i < nb; ++i) {
        int a, b;
        shape_ab(*cfg, chunkShape[(size_t)(i * fi.nch)], &a, &b);
        block_start[i] = start;
        block_a[i] = a;
        block_b[i] = b;
        start += a;
    }
    std::copy(chunkOff.begin(), chunkOff.end(), chunk_offset);
    return MRC_OK;
}

int mrc_get_decode_ms(mrc_handle* h, double* ms) {
    if (!h || !ms) return MRC_ERR_INVALID;
    for (int i = 0; i < 4; ++i) ms[i] = h->dec.ms[i];
    return MRC_OK;
}

}  // extern "C"
