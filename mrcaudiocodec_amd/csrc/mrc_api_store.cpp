// C ABI, resident `.pac` store (include/mrc_hip.h: mrc_pac_store_*): files uploaded once, sample windows decoded into the
// caller's device memory.
//
// create: pac_plan_scan -- the host plan of mrc_decode_pac_pcm16, one scan in the tree -- gives every file's chunks, block
// shapes and positions; the bytes go to the device in one copy and never cross PCIe again.
//
// decode_window, per slab of whole items:
//   needed blocks   block i of the item's file iff p_i < start + window + L and p_i + a_i + b_i > start + L (p_i its position
//                   in the padded plane, L = n_mdct_lines): positions increase, so the end is a binary search, and as
//                   a + b <= 2 L so is a point before which no block can reach the window; the few blocks behind it are
//                   tested one by one.
//   margin planes   each item that needs a block gets a float64 plane of window + 4 L samples per decoded channel, the
//                   window at [2 L, 2 L + window): a needed block starts at 2 L + p_i - (start + L), which lies in
//                   (2 L - (a + b), 2 L + window), so every needed block fits with decode_kernel unchanged.  Each window
//                   sample receives exactly the contributions it receives in the whole-file decode (a block that
//                   contributes to it overlaps the window, hence is needed), added to zero: the same bits.
//   groups          the needed (block, channel)s of ALL items of the slab are slots of at most eight (shape, kind) groups:
//                   one unpack_dense_kernel launch, at most eight decode_kernel launches.  A block's kind is its position
//                   in its file: joint for all but the last block of a stereo file of more than one block.
//   window_out_kernel  planes -> out [item][channel][t] in the caller's format (mrc_kernels_store.hip).
// The plan entries point into the resident bytes; what is uploaded per slab is the plan alone.  Staging offsets, slot counts,
// the parse step and the walk over the groups are the whole-file decode's (StageLayout, PacGroupCounts::add_block, pac_parse with
// the resident bytes as what the entries point into, pac_for_groups / decode_groups); a bad chunk's file is found from the
// index's file bases like everywhere else.
//
// decode_window_reduced, rate divisor D = 2 or 4 (D = 1: the call above): the same plan with every length divided by D --
// L / D, p_i / D, (a_i + b_i) / D, planes of window + 4 L / D, start and window in reduced samples -- exact, because every
// block length and position is a multiple of n_short and D divides n_short (else the shapes have no reduced form and the
// call is refused).  The parser is untouched (a chunk's bits are sequential: every mantissa is parsed); decode_reduced_kernel
// dequantises the first 1 / D of a block's lines and runs the inverse transform of the shape (a, b) / D.  One function,
// decode_windows, holds the arithmetic for every D.
//
// decode_window_mix, one channel of every item (left, right or the mid (L + R) / 2): the same plan with ONE plane per item
// and one workgroup per needed block (decode_mix_kernel, its selector an argument).  A joint block keeps its slot of two
// chunks -- the M/S switches and both streams are needed even for left.  The non-joint last block of a stereo file is one
// single slot for left / right (the other channel's chunk is not in the plan) and for mid a PAIR: two neighbouring slots
// of the non-joint group, which laid side by side are one slot of two streams, the group's pairs in front of its single
// slots so that a workgroup finds its slot from its index alone.  pac_plan_layout sees slot counts as ever.
#include "mrc_handle.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>

using namespace mrc;

namespace {

const char* const kWin = "mrc_pac_store_decode_window";
const char* const kWinReduced = "mrc_pac_store_decode_window_reduced";
const char* const kWinMix = "mrc_pac_store_decode_window_mix";
constexpr int kNoMix = -1;                           // decode_windows: every channel of a file into a plane of its own

int store_alive(mrc_pac_store* s, const char* fn) {
    if (!s) return fail(nullptr, MRC_ERR_INVALID, std::string(fn) + ": null store");
    if (!s->h) return fail(nullptr, MRC_ERR_INVALID, std::string(fn) + ": the store's handle has been destroyed");
    return MRC_OK;
}

struct Need { int64_t item, file, block; };          // item: index in the slab

// the blocks of file f that a window of `window` samples at `start` overlaps, appended to out as (item, f, block); start
// and window count samples at 1 / D of the file's rate, where block i covers [p_i / D, (p_i + a_i + b_i) / D)
void needed_blocks(const mrc_pac_store& s, const mrc_config& cfg, int D, int64_t item, int64_t f, int64_t start, int64_t window,
                   std::vector<Need>* out) {
    const int64_t L = cfg.n_mdct_lines / D, nb = s.index.nBlocks(f);
    // no block reaches past the file's extent or before 0 (compared without forming start + window where start is extreme)
    if (nb == 0 || start >= (s.index.files[(size_t)f].extent - cfg.n_mdct_lines) / D ||
        (start < 0 && -(start + 1) >= window + L - 1))
        return;
    const int64_t* p = s.blockStart.data() + s.firstBlock[(size_t)f];
    const int64_t lo = (start + L) * D, hi = (start + window + L) * D;      // in the file's own samples: p_i is a multiple of D
    const int64_t first = std::upper_bound(p, p + nb, lo - 2 * L * D) - p, end = std::lower_bound(p, p + nb, hi) - p;
    for (int64_t i = first; i < end; ++i) {
        int a, b;
        shape_ab(cfg, s.index.shape(f, i), &a, &b);
        if (p[i] + a + b > lo) out->push_back(Need{item, f, i});
    }
}

}  // namespace

extern "C" {

int mrc_pac_store_create(mrc_handle* h, int64_t n_files, const uint8_t* buf, const int64_t* file_offset,
                         mrc_pac_store** out) {
    if (!h) return MRC_ERR_INVALID;
    if (out) *out = nullptr;
    if (!out) return fail(h, MRC_ERR_INVALID, "mrc_pac_store_create: bad argument");
    MRC_TRY(check_file_list(h, "mrc_pac_store_create", n_files, buf, file_offset));
    std::unique_ptr<mrc_pac_store> s(new (std::nothrow) mrc_pac_store());
    if (!s) return fail(h, MRC_ERR_NOMEM, "mrc_pac_store_create: out of host memory");
    MRC_TRY(pac_plan_scan(h, "mrc_pac_store_create", n_files, buf, file_offset, &s->index));
    s->firstBlock.assign((size_t)n_files + 1, 0);
    for (int64_t f = 0; f < n_files; ++f) {
        int64_t start = 0;
        for (int64_t i = 0; i < s->index.nBlocks(f); ++i) {
            int a, b;
            shape_ab(h->cfg, s->index.shape(f, i), &a, &b);
            s->blockStart.push_back(start);
            start += a;
        }
        s->firstBlock[(size_t)f + 1] = (int64_t)s->blockStart.size();
    }
    s->nBytes = n_files ? file_offset[n_files] - file_offset[0] : 0;
    MRC_TRY(ensure_decode_consts(h));
    MRC_HIP(h, s->bytes.reserve(std::max<size_t>((size_t)s->nBytes, 256)));
    if (s->nBytes) MRC_HIP(h, hipMemcpy(s->bytes.p, buf + file_offset[0], (size_t)s->nBytes, hipMemcpyHostToDevice));
    s->h = h;
    h->stores.push_back(s.get());
    *out = s.release();
    return MRC_OK;
}

void mrc_pac_store_destroy(mrc_pac_store* s) {
    if (!s) return;
    if (mrc_handle* h = s->h) {
        h->stores.erase(std::remove(h->stores.begin(), h->stores.end(), s), h->stores.end());
        (void)hipSetDevice(h->device);
        if (h->stream) (void)hipStreamSynchronize(h->stream);
    }
    delete s;
}

int mrc_pac_store_info(mrc_pac_store* s, int64_t* n_files, int32_t* n_channels, int64_t* n_samples, int64_t* n_blocks,
                       int64_t* device_bytes) {
    MRC_TRY(store_alive(s, "mrc_pac_store_info"));
    const int64_t n = (int64_t)s->index.files.size(), L = s->h->cfg.n_mdct_lines;
    if (n_files) *n_files = n;
    for (int64_t f = 0; f < n; ++f) {
        const PacFilePlan& fi = s->index.files[(size_t)f];
        if (n_channels) n_channels[f] = fi.nch;
        if (n_samples) n_samples[f] = std::max<int64_t>(0, fi.total - L);
        if (n_blocks) n_blocks[f] = s->index.nBlocks(f);
    }
    if (device_bytes) *device_bytes = (int64_t)s->bytes.cap;
    return MRC_OK;
}

}  // extern "C"

namespace {

// all decode_window calls: fn the entry point's name, D the rate divisor (1: full rate, decode_kernel), mixArg null or the
// caller's MRC_MIX_* (one plane per item, decode_mix_kernel; n_channels_out is then 1)
int decode_windows(mrc_pac_store* s, const char* fn, int D, const int* mixArg, int64_t n_items, const int64_t* file, const int64_t* start,
                   int64_t window, int n_channels_out, int format, void* out, void* stream) {
    MRC_TRY(store_alive(s, fn));
    mrc_handle* h = s->h;
    const mrc_config& cfg = h->cfg;
    const std::string w = fn;
    for (int i = 0; i < 4; ++i) { s->stats[i] = 0; s->ms[i] = 0.0; }
    const int mix = mixArg ? *mixArg : kNoMix;
    if (mixArg && mix != MRC_MIX_MID && mix != MRC_MIX_LEFT && mix != MRC_MIX_RIGHT)
        return fail(h, MRC_ERR_INVALID, w + ": mix " + std::to_string(mix) + " is not MRC_MIX_MID (0), MRC_MIX_LEFT (1) or MRC_MIX_RIGHT (2)");
    if (D != 1 && D != 2 && D != 4) return fail(h, MRC_ERR_INVALID, w + ": rate_divisor " + std::to_string(D) + " is not 1, 2 or 4");
    for (int sh = 0; D > 1 && sh < 4; ++sh) {
        int a, b;
        shape_ab(cfg, sh, &a, &b);
        const std::string refusal = synth_shape_refusal(a, b, D);
        if (!refusal.empty()) return fail(h, MRC_ERR_INVALID, w + ": " + refusal);
    }
    const int64_t nFiles = (int64_t)s->index.files.size(), L = cfg.n_mdct_lines / D;      // L: the margin unit, reduced samples
    if (n_items < 0) return fail(h, MRC_ERR_INVALID, w + ": n_items < 0");
    if (window < 0 || window > ((int64_t)1 << 40)) return fail(h, MRC_ERR_INVALID, w + ": window must lie in [0, 2^40]");
    if (n_channels_out != 1 && n_channels_out != 2) return fail(h, MRC_ERR_INVALID, w + ": n_channels_out must be 1 or 2");
    if (format != MRC_WINDOW_PCM16 && format != MRC_WINDOW_F32 && format != MRC_WINDOW_F64)
        return fail(h, MRC_ERR_INVALID, w + ": unknown format " + std::to_string(format));
    if (n_items > 0 && (!file || !start)) return fail(h, MRC_ERR_INVALID, w + ": file or start is NULL");
    if (n_items > 0 && window > 0 && !out) return fail(h, MRC_ERR_INVALID, w + ": out is NULL");
    for (int64_t k = 0; k < n_items; ++k) {
        if (file[k] < 0 || file[k] >= nFiles)
            return fail(h, MRC_ERR_INVALID, w + ": file[" + std::to_string(k) + "] = " + std::to_string(file[k]) + " is outside the store's " +
                                                std::to_string(nFiles) + " files");
        if (mix == kNoMix && s->index.files[(size_t)file[k]].nch > n_channels_out)
            return fail(h, MRC_ERR_INVALID, w + ": item " + std::to_string(k) + ": file " + std::to_string(file[k]) +
                                                " is stereo, the call asks for one channel");
    }
    if (n_items == 0 || window == 0) return MRC_OK;

    MRC_TRY(ensure_decode_consts(h));
    DecodeBufs& d = h->dec;
    StoreBufs& b = h->store;
    MRC_HIP(h, b.ev.create());
    hipStream_t st = pick_stream(h, stream);
    DrainGuard drain{{st, nullptr, nullptr}};
    const size_t elem = format == MRC_WINDOW_PCM16 ? 2 : format == MRC_WINDOW_F32 ? 4 : 8;
    const int64_t planeLen = window + 4 * L, tiles = (window + 255) / 256;
    const int64_t slab = h->storeSlabSamples, itemCap = std::max<int64_t>(1, 0x7fffffffLL / (tiles * n_channels_out));

    std::vector<Need> needs;
    std::vector<WindowItem> items;
    // chunks of a needed non-joint block that are parsed: all of the file's, but under left / right the one asked for
    const auto lastChunks = [mix](int nch) { return mix == MRC_MIX_LEFT || mix == MRC_MIX_RIGHT ? 1 : nch; };
    PacPlan pl;                                              // (its group fields: the slab's slots)
    for (int64_t first = 0, last; first < n_items; first = last) {
        last = first + 1;
        while (last < n_items && last - first < itemCap && (slab == 0 || (last - first + 1) * window <= slab)) ++last;
        const int64_t nSlab = last - first;
        unsigned char* outSlab = (unsigned char*)out + (size_t)first * n_channels_out * window * elem;
        s->stats[2] += 1;

        // ---- the slab's needed blocks, its items and planes
        needs.clear();
        items.assign((size_t)nSlab, WindowItem{0, 0, 0, 1, 0});
        int64_t planeDoubles = 0;
        for (int64_t k = 0; k < nSlab; ++k) {
            const int64_t f = file[first + k];
            const size_t before = needs.size();
            needed_blocks(*s, cfg, D, k, f, start[first + k], window, &needs);
            if (needs.size() == before) continue;            // all zeros: its plane does not exist
            const PacFilePlan& fi = s->index.files[(size_t)f];
            const int nPlanes = mix == kNoMix ? fi.nch : 1;
            items[(size_t)k] = WindowItem{planeDoubles, start[first + k], std::max<int64_t>(0, fi.total - cfg.n_mdct_lines) / D, nPlanes, 0};
            planeDoubles += nPlanes * planeLen;
        }
        if (needs.empty()) {                                 // nothing to decode: zeros, no launch
            MRC_HIP(h, hipMemsetAsync(outSlab, 0, (size_t)nSlab * n_channels_out * window * elem, st));
            continue;
        }
        pl.clear_counts();
        // mid: the two chunks of a stereo file's last block are a PAIR of neighbouring slots of the non-joint group, the
        // pairs in front of the group's single slots (launch_decode_mix)
        int64_t nPairs[kUnpackGroups] = {};
        for (const Need& n : needs) {
            const int nch = lastChunks(s->index.files[(size_t)n.file].nch), sh = s->index.shape(n.file, n.block);
            const bool joint = n.block < s->index.nJoint(n.file);
            pl.add_block(sh, joint, nch);
            if (!joint && mix == MRC_MIX_MID && nch == 2) nPairs[sh * 2 + 1] += 1;
        }
        MRC_TRY(pac_plan_layout(h, fn, &pl));
        const HostShape* reduced[4] = {};
        for (int sh = 0; D > 1 && sh < 4; ++sh)
            if (pl.hs[sh]) MRC_TRY(get_synth_shape(h, pl.hs[sh]->dev.a, pl.hs[sh]->dev.b, D, &reduced[sh]));
        const int64_t nChunks = pl.nEntries();

        // ---- staging (one H2D copy): plan | groups | block offsets | items
        StageLayout lay(256);
        const size_t oPlan = lay.add<UnpackPlanEntry>(nChunks), oGroups = lay.add<UnpackGroupDev>(kUnpackGroups),
                     oOffs = lay.add<long long>(pl.totalSlots), oItems = lay.add<WindowItem>(nSlab), inTotal = lay.total();
        MRC_HIP(h, b.pinIn.reserve(inTotal));
        MRC_HIP(h, b.in.reserve(inTotal));
        MRC_HIP(h, b.groups.reserve(std::max<size_t>(pl.gBytes, 256)));
        MRC_HIP(h, b.planes.reserve(sizeof(double) * (size_t)planeDoubles));
        unsigned char* pin = (unsigned char*)b.pinIn.p;
        UnpackPlanEntry* plan = (UnpackPlanEntry*)(pin + oPlan);
        UnpackGroupDev* gd = (UnpackGroupDev*)(pin + oGroups);
        long long* offs = (long long*)(pin + oOffs);
        std::memcpy(pin + oItems, items.data(), sizeof(WindowItem) * nSlab);
        pac_plan_group_descs(d, pl, gd, b.groups.as<unsigned char>());
        int64_t catPos[2 * kUnpackGroups], slotNext[kUnpackGroups] = {}, pairNext[kUnpackGroups] = {};
        for (int64_t k = 0, q = 0; k < 2 * kUnpackGroups; q += pl.nCat[k], ++k) catPos[k] = q;
        for (int g = 0; g < kUnpackGroups; ++g) slotNext[g] = 2 * nPairs[g];      // (joint groups, and every group without mid: 0)
        for (const Need& n : needs) {
            const PacFilePlan& fi = s->index.files[(size_t)n.file];
            const WindowItem& it = items[(size_t)n.item];
            const int64_t c0 = fi.firstChunk + n.block * fi.nch;
            const int sh = s->index.chunkShape[(size_t)c0];
            // the block's place in the item's plane: its position in the file's padded plane, the window's start at 2 L
            const int64_t at = it.plane + 2 * L + s->blockStart[(size_t)(s->firstBlock[(size_t)n.file] + n.block)] / D - (it.start + L);
            if (n.block < s->index.nJoint(n.file)) {
                const int g = sh * 2, slot = (int)slotNext[g]++;
                for (int ch = 0; ch < 2; ++ch)
                    plan[catPos[sh * 4 + ch]++] = UnpackPlanEntry{s->index.chunkOff[(size_t)c0 + ch], g * 2 + ch, slot};
                offs[pl.slotBase[g] + slot] = at;
            } else {
                const int g = sh * 2 + 1, nParsed = lastChunks(fi.nch), ch0 = fi.nch == 2 && mix == MRC_MIX_RIGHT ? 1 : 0;
                const bool pair = mix == MRC_MIX_MID && fi.nch == 2;
                if (pair) offs[pl.slotBase[g] + pairNext[g] / 2] = at;
                for (int ch = ch0; ch < ch0 + nParsed; ++ch) {
                    const int slot = (int)(pair ? pairNext[g]++ : slotNext[g]++);
                    plan[catPos[sh * 4 + 2]++] = UnpackPlanEntry{s->index.chunkOff[(size_t)c0 + ch], g * 2, slot};
                    // a single slot's workgroup comes after the group's pairs; without a mix a channel has a plane of its own
                    if (!pair) offs[pl.slotBase[g] + slot - nPairs[g]] = at + (mix == kNoMix ? ch * planeLen : 0);
                }
            }
        }
        s->stats[0] += nChunks;
        s->stats[3] += (int64_t)inTotal;

        // ---- device: the parse step (the plan entries point into the resident bytes), then one launch per group with slots
        unsigned char* din = b.in.as<unsigned char>();
        MRC_TRY(pac_parse(h, fn, s->index.fileBase,
                          PacParse{pin, din, inTotal, oPlan, oGroups, nChunks, s->bytes.as<uint8_t>(), s->nBytes,
                                   {b.ev[0], b.ev[1], b.ev[2]}, st}));
        double* x = b.planes.as<double>();
        MRC_HIP(h, hipEventRecord(b.ev[3], st));
        MRC_HIP(h, hipMemsetAsync(x, 0, sizeof(double) * (size_t)planeDoubles, st));
        const int64_t* offsDev = (const int64_t*)(din + oOffs);
        if (mix == kNoMix && D == 1) MRC_TRY(decode_groups(h, pl, gd, offsDev, x, planeLen, st));
        else
            MRC_TRY(pac_for_groups(h, pl, gd, offsDev, [&](int g, const UnpackGroupDev& G, const int64_t* o) {
                const DevShape& F = pl.hs[g / 2]->dev;
                if (mix != kNoMix)
                    return launch_decode_mix(F, D == 1 ? nullptr : &reduced[g / 2]->dev, pl.nSlots[g] - nPairs[g], G.joint,
                                             mix == MRC_MIX_MID ? 2 : mix == MRC_MIX_LEFT ? 0 : 1, nPairs[g], G.oscale,
                                             G.joint ? G.ms : nullptr, G.sf, G.ba, G.mant, o, x, st);
                return launch_decode_reduced(F, reduced[g / 2]->dev, pl.nSlots[g], G.joint ? 2 : 1, G.oscale,
                                             G.joint ? G.ms : nullptr, G.sf, G.ba, G.mant, o, x,
                                             G.joint ? x + planeLen : nullptr, st);
            }));
        s->stats[1] += pl.groupsUsed();
        MRC_HIP(h, hipEventRecord(b.ev[4], st));
        MRC_HIP(h, launch_window_out(nSlab, (const WindowItem*)(din + oItems), window, n_channels_out, format, (int)L, x,
                                     outSlab, st));
        MRC_HIP(h, hipEventRecord(b.ev[5], st));
        MRC_HIP(h, hipStreamSynchronize(st));                // (the staging is written again by the next slab)
        const int span[4][2] = {{0, 1}, {1, 2}, {3, 4}, {4, 5}};
        for (int i = 0; i < 4; ++i) {
            double ms = 0.0;
            MRC_HIP(h, b.ev.elapsed(span[i][0], span[i][1], &ms));
            s->ms[i] += ms;
        }
    }
    MRC_HIP(h, hipStreamSynchronize(st));
    return MRC_OK;
}

}  // namespace

extern "C" {

int mrc_pac_store_decode_window(mrc_pac_store* s, int64_t n_items, const int64_t* file, const int64_t* start, int64_t window,
                                int n_channels_out, int format, void* out, void* stream) {
    return decode_windows(s, kWin, 1, nullptr, n_items, file, start, window, n_channels_out, format, out, stream);
}

int mrc_pac_store_decode_window_reduced(mrc_pac_store* s, int rate_divisor, int64_t n_items, const int64_t* file,
                                        const int64_t* start, int64_t window, int n_channels_out, int format, void* out,
                                        void* stream) {
    return decode_windows(s, kWinReduced, rate_divisor, nullptr, n_items, file, start, window, n_channels_out, format, out, stream);
}

int mrc_pac_store_decode_window_mix(mrc_pac_store* s, int rate_divisor, int mix, int64_t n_items, const int64_t* file,
                                    const int64_t* start, int64_t window, int format, void* out, void* stream) {
    return decode_windows(s, kWinMix, rate_divisor, &mix, n_items, file, start, window, 1, format, out, stream);
}

int mrc_synthesis_shape(int a, int b, int rate_divisor) {
    const std::string refusal = synth_shape_refusal(a, b, rate_divisor);
    return refusal.empty() ? MRC_OK : fail(nullptr, MRC_ERR_INVALID, "mrc_synthesis_shape: " + refusal);
}

int mrc_pac_store_stats(mrc_pac_store* s, int64_t* stats, double* ms) {
    MRC_TRY(store_alive(s, "mrc_pac_store_stats"));
    for (int i = 0; i < 4; ++i) {
        if (stats) stats[i] = s->stats[i];
        if (ms) ms[i] = s->ms[i];
    }
    return MRC_OK;
}

}  // extern "C"
