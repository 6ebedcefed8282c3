// Noise-to-mask ratio of whole `.pac` files against their source, on the device in one call (mrc_pac_nmr).
//
// The host plan is decode's (pac_plan_scan / pac_plan_groups / pac_plan_fill in mrc_api_decode.cpp): headers, parameter
// checks, chunks with their shape bits, block groups and positions.  Block i of a file covers [p_i, p_i + a_i + b_i) of
// the channel's padded source (n_mdct_lines zeros, the caller's samples, zeros), p_i = a_0 + ... + a_{i-1} -- where
// decode_kernel adds the block.  One H2D copy carries the bytes, the plan and the sources (each distinct source plane
// once: the rungs of a ladder name the same samples); then on the device:
//   nmr_pad_kernel          padded int16 planes;
//   unpack_dense_kernel     the chunks into the dense per-(shape, kind) arrays, unchanged;
//   launch_mdct, launch_smr per block shape over every distinct (plane, position) of the call: X and the masked
//                           threshold T (smr_kernel's generic mode, the one that writes thresholds);
//   nmr_band_kernel         per (block, channel): the decoded lines, noise_j, mask_j, r_j;
//   nmr_file_kernel         per file: max r, sum of b * mean r, disturbed blocks;
// and one D2H copy.  The dB values are formed on the host from the file sums.
//
// mrc_pac_nmr reads as the list of its steps: nmr_refusals, nmr_source_planes, nmr_stage_layout (a StageLayout each way),
// nmr_fill_stage (entries and distinct analyses, written into the staging), nmr_device (pac_parse, then the kernels above),
// nmr_results.
#include "mrc_handle.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <unordered_map>

using namespace mrc;

namespace {

struct AnaKey {
    int64_t plane, pos;
    int shape;
    bool operator==(const AnaKey& o) const { return plane == o.plane && pos == o.pos && shape == o.shape; }
};
struct AnaHash {
    size_t operator()(const AnaKey& k) const {
        uint64_t x = (uint64_t)k.plane * 0x9E3779B97F4A7C15ull ^ ((uint64_t)k.pos << 2 | (uint64_t)k.shape);
        x ^= x >> 31;
        x *= 0xBF58476D1CE4E5B9ull;
        return (size_t)(x ^ (x >> 29));
    }
};
struct PlaneKey {
    uintptr_t p;
    int64_t frames;
    bool operator==(const PlaneKey& o) const { return p == o.p && frames == o.frames; }
};
struct PlaneHash {
    size_t operator()(const PlaneKey& k) const { return std::hash<uintptr_t>()(k.p) * 31 + std::hash<int64_t>()(k.frames); }
};

const char* const kFn = "mrc_pac_nmr";

// the caller's arguments, as the steps below pass them on
struct NmrCall {
    int64_t n_files;
    const uint8_t* buf;
    const int64_t* file_offset;
    const int16_t* src;
    const int64_t *src_offset, *src_stride, *src_frames;
    double *nmr_max_db, *nmr_total_db;
    int64_t *disturbed_blocks, *n_blocks, *entry_offset, entry_cap;
    int32_t* entry_shape;
    double *band_noise, *band_mask;
    bool detail() const { return band_noise != nullptr; }
    int64_t nEntries() const { return entry_offset[n_files]; }
    int64_t inBytes() const { return file_offset[n_files] - file_offset[0]; }
};
struct NmrPlanes {
    std::vector<NmrPlane> planes;
    std::vector<const int16_t*> planeSrc;        // per plane: its first sample in the caller's memory
    std::vector<int64_t> fileChPlane;            // [file][2]: the plane of the file's channel
    int64_t planeTotal = 0, srcTotal = 0, maxLen = 0;   // padded samples on the device; samples uploaded; longest plane
};
struct NmrWork {
    std::vector<NmrEntry> ent[4];                // per block shape: one entry per (block, channel)
    std::vector<long long> anaOff[4];            // ... and the distinct (plane, position)s to analyse
    size_t anaBytes[4] = {}, anaTotal = 0, anaRows = 0;   // where a shape's X / T rows start; their bytes; rows of all shapes
};
// the one copy in and the one copy out, field by field
struct NmrStage {
    size_t oBytes, oPlan, oGroups, oEnt[4], oAna[4], oEntryStart, oNch, oPlanes, oSrc, inTotal;
    size_t oFiles, oNoise, oMask, bandBytes, outTotal;
};

// Refusals and entry offsets: everything that can be said from the arguments and the host plan (decode's; host only)
// before any device work -- the argument checks, the files' headers and chunks, a stereo file whose source planes overlap,
// and entry_cap (NOMEM).  Fills n_blocks and entry_offset: one entry per (block, channel) = per chunk.
int nmr_refusals(mrc_handle* h, const NmrCall& c, PacPlan* pl) {
    if (!c.src_offset || !c.src_stride || !c.src_frames || !c.nmr_max_db || !c.nmr_total_db || !c.disturbed_blocks ||
        !c.n_blocks || !c.entry_offset || c.entry_cap < 0 || (c.band_noise == nullptr) != (c.band_mask == nullptr) ||
        // (this call words the file list's null checks its own way; check_file_list's own never fire)
        c.n_files < 0 || !c.file_offset || (c.n_files > 0 && !c.buf))
        return fail(h, MRC_ERR_INVALID, "mrc_pac_nmr: bad argument (band_noise and band_mask go together)");
    char msg[200];
    c.entry_offset[0] = 0;
    MRC_TRY(check_file_list(h, kFn, c.n_files, c.buf, c.file_offset));
    for (int64_t f = 0; f < c.n_files; ++f)
        if (c.src_offset[f] < 0 || c.src_stride[f] < 0 || c.src_frames[f] < 0 || (c.src_frames[f] > 0 && !c.src)) {
            std::snprintf(msg, sizeof msg, "mrc_pac_nmr: file %lld: negative source offset, stride or frame count, or no source",
                          (long long)f);
            return fail(h, MRC_ERR_INVALID, msg);
        }
    if (c.n_files == 0) return MRC_OK;
    MRC_TRY(pac_plan_scan(h, kFn, c.n_files, c.buf, c.file_offset, pl));
    for (int64_t f = 0; f < c.n_files; ++f) {
        const PacFilePlan& fi = pl->files[(size_t)f];
        if (fi.nch == 2 && c.src_stride[f] < c.src_frames[f]) {
            std::snprintf(msg, sizeof msg, "mrc_pac_nmr: file %lld is stereo and its source stride %lld is below its %lld frames",
                          (long long)f, (long long)c.src_stride[f], (long long)c.src_frames[f]);
            return fail(h, MRC_ERR_INVALID, msg);
        }
        c.n_blocks[f] = pl->nBlocks(f);
        c.entry_offset[f + 1] = c.entry_offset[f] + fi.nChunks;
    }
    if ((c.detail() || c.entry_shape) && c.nEntries() > c.entry_cap) {
        std::snprintf(msg, sizeof msg, "mrc_pac_nmr: the files hold %lld entries, entry_cap is %lld", (long long)c.nEntries(),
                      (long long)c.entry_cap);
        return fail(h, MRC_ERR_NOMEM, msg);
    }
    return MRC_OK;
}

// Source planes: one per distinct (first sample, frame count) -- the rungs of a ladder name the same samples, which then
// travel and are analysed once -- as long as the longest file that reads it.  A plane is n_mdct_lines zeros, the samples a
// block can reach, zeros; its length is rounded up to 64 samples on the device.
NmrPlanes nmr_source_planes(const NmrCall& c, const PacPlan& pl, int L) {
    NmrPlanes P;
    std::unordered_map<PlaneKey, int64_t, PlaneHash> planeOf;
    P.fileChPlane.assign((size_t)c.n_files * 2, -1);
    for (int64_t f = 0; f < c.n_files; ++f) {
        const PacFilePlan& fi = pl.files[(size_t)f];
        for (int ch = 0; ch < fi.nch; ++ch) {
            const int16_t* p0 = c.src ? c.src + c.src_offset[f] + ch * c.src_stride[f] : nullptr;
            const PlaneKey key{(uintptr_t)p0, c.src_frames[f]};
            auto it = planeOf.find(key);
            if (it == planeOf.end()) {
                it = planeOf.emplace(key, (int64_t)P.planes.size()).first;
                P.planes.push_back(NmrPlane{0, 0, c.src_frames[f], 0});
                P.planeSrc.push_back(p0);
            }
            NmrPlane& q = P.planes[(size_t)it->second];
            q.len = std::max<long long>(q.len, fi.extent);
            P.fileChPlane[(size_t)(2 * f + ch)] = it->second;
        }
    }
    for (NmrPlane& q : P.planes) {
        q.frames = std::min<long long>(q.frames, std::max<long long>(0, q.len - L));   // samples a block reads
        q.dst = P.planeTotal;
        q.src = P.srcTotal;
        P.planeTotal += (q.len + 63) & ~63LL;
        P.srcTotal += q.frames;
        P.maxLen = std::max<int64_t>(P.maxLen, q.len);
    }
    return P;
}

// Staging, the layout.  In (one H2D copy): bytes | plan | groups | entries [4 shapes] | analysis offsets [4 shapes] |
// entryStart [n + 1] | nch [n] | planes | source samples.  Entries per shape are known from the group slot counts: a joint
// slot is two entries, a non-joint slot one; there are at most as many analyses.  Out (one D2H copy): per-file sums | band
// noise | band mask -- the bands only travel when asked for.
NmrStage nmr_stage_layout(const NmrCall& c, const PacPlan& pl, const NmrPlanes& P) {
    NmrStage S;
    StageLayout in(256), out(256);
    const auto perShape = [&](int s) { return (size_t)(2 * pl.nSlots[2 * s] + pl.nSlots[2 * s + 1]); };
    S.oBytes = in.add((size_t)c.inBytes());
    S.oPlan = in.add<UnpackPlanEntry>(pl.nChunks());
    S.oGroups = in.add<UnpackGroupDev>(kUnpackGroups);
    for (int s = 0; s < 4; ++s) S.oEnt[s] = in.add<NmrEntry>(perShape(s));
    for (int s = 0; s < 4; ++s) S.oAna[s] = in.add<long long>(perShape(s));
    S.oEntryStart = in.add<long long>(c.n_files + 1);
    S.oNch = in.add<int>(c.n_files);
    S.oPlanes = in.add<NmrPlane>(P.planes.size());
    S.oSrc = in.add<int16_t>((size_t)P.srcTotal);
    S.inTotal = in.total();
    S.bandBytes = sizeof(double) * kMaxBands * (size_t)c.nEntries();
    S.oFiles = out.add<double>(4 * c.n_files);
    S.oNoise = out.add(S.bandBytes);
    S.oMask = out.total();
    S.outTotal = c.detail() ? S.oMask + S.bandBytes : S.oNoise;
    return S;
}

// Entries and the distinct analyses per block shape, written into the staging `pin` with everything else that travels:
// pac_plan_fill's visitor names every (block, channel) once; a (plane, position, shape) seen before is analysed once.
NmrWork nmr_fill_stage(mrc_handle* h, const NmrCall& c, const PacPlan& pl, const NmrPlanes& P, const NmrStage& S,
                       unsigned char* pin) {
    NmrWork W;
    std::unordered_map<AnaKey, int64_t, AnaHash> anaOf;
    anaOf.reserve((size_t)c.nEntries());
    auto add_entry = [&](int64_t f, int64_t i, int g, int slot, int ch, int64_t start) {
        const int s = g / 2;
        int a, b;
        shape_ab(h->cfg, s, &a, &b);
        const int64_t plane = P.fileChPlane[(size_t)(2 * f + ch)];
        auto it = anaOf.find(AnaKey{plane, start, s});
        if (it == anaOf.end()) {
            it = anaOf.emplace(AnaKey{plane, start, s}, (int64_t)W.anaOff[s].size()).first;
            W.anaOff[s].push_back(P.planes[(size_t)plane].dst + start);
        }
        const int64_t e = c.entry_offset[f] + i * pl.files[(size_t)f].nch + ch;
        W.ent[s].push_back(NmrEntry{e, it->second, g, slot, ch, b});
    };
    copy_host(pin + S.oBytes, c.buf + c.file_offset[0], (size_t)c.inBytes());
    pac_plan_fill(h->cfg, h->dec, pl, (UnpackPlanEntry*)(pin + S.oPlan), (UnpackGroupDev*)(pin + S.oGroups),
                  h->nmr.groups.as<unsigned char>(), [&](int64_t f, int64_t i, int g, int slot, int ch, int64_t start) {
                      if (g & 1) add_entry(f, i, g, slot, ch, start);                 // non-joint: one chunk, one entry
                      else { add_entry(f, i, g, slot, 0, start); add_entry(f, i, g, slot, 1, start); }
                  });
    StageLayout ana(256);
    for (int s = 0; s < 4; ++s) {
        std::memcpy(pin + S.oEnt[s], W.ent[s].data(), sizeof(NmrEntry) * W.ent[s].size());
        std::memcpy(pin + S.oAna[s], W.anaOff[s].data(), sizeof(long long) * W.anaOff[s].size());
        W.anaBytes[s] = ana.add<double>(W.anaOff[s].size() * (size_t)h->dec.bands.halfN[s]);
        W.anaRows += W.anaOff[s].size();
    }
    W.anaTotal = ana.total();
    long long* entryStart = (long long*)(pin + S.oEntryStart);
    int* nchDev = (int*)(pin + S.oNch);
    for (int64_t f = 0; f <= c.n_files; ++f) entryStart[f] = c.entry_offset[f];
    for (int64_t f = 0; f < c.n_files; ++f) nchDev[f] = pl.files[(size_t)f].nch;
    std::memcpy(pin + S.oPlanes, P.planes.data(), sizeof(NmrPlane) * P.planes.size());
    for (size_t q = 0; q < P.planes.size(); ++q)
        if (P.planes[q].frames)
            copy_host(pin + S.oSrc + sizeof(int16_t) * P.planes[q].src, P.planeSrc[q], sizeof(int16_t) * P.planes[q].frames);
    return W;
}

// Device: the parse step (pac_parse: the plan entries point into the staging's own bytes), nmr_pad_kernel, the source
// analysis per shape over its distinct (plane, position)s (launch_nmr_source: X and the masked threshold T),
// nmr_band_kernel per shape over its entries, nmr_file_kernel, and the one copy back into NmrBufs::pinOut.
int nmr_device(mrc_handle* h, const NmrCall& c, const PacPlan& pl, const NmrPlanes& P, const NmrWork& W, const NmrStage& S) {
    NmrBufs& nb = h->nmr;
    const bool detail = c.detail();
    MRC_HIP(h, nb.planes.reserve(std::max<size_t>(sizeof(int16_t) * P.planeTotal, 256)));
    MRC_HIP(h, nb.lines.reserve(std::max<size_t>(W.anaTotal, 256)));
    MRC_HIP(h, nb.thresh.reserve(std::max<size_t>(W.anaTotal, 256)));
    MRC_HIP(h, nb.oscale.reserve(std::max<size_t>(sizeof(int) * W.anaRows, 256)));
    MRC_HIP(h, nb.smr.reserve(std::max<size_t>(sizeof(double) * kMaxBands * W.anaRows, 256)));
    MRC_HIP(h, nb.stat.reserve(std::max<size_t>(sizeof(double) * 2 * c.nEntries(), 256)));
    MRC_HIP(h, nb.out.reserve(S.outTotal));
    MRC_HIP(h, nb.pinOut.reserve(S.outTotal));

    hipStream_t st = h->stream;
    unsigned char* din = nb.in.as<unsigned char>();
    MRC_TRY(pac_parse(h, kFn, pl.fileBase,
                      PacParse{nb.pinIn.p, din, S.inTotal, S.oPlan, S.oGroups, pl.nChunks(), din + S.oBytes, c.inBytes(),
                               {nb.ev[0], nb.ev[1], nb.ev[2]}, st}));
    short* dPlanes = nb.planes.as<short>();
    MRC_HIP(h, launch_nmr_pad((int64_t)P.planes.size(), (const NmrPlane*)(din + S.oPlanes), P.maxLen, h->cfg.n_mdct_lines,
                              (const short*)(din + S.oSrc), dPlanes, st));
    unsigned char* dLines = nb.lines.as<unsigned char>();
    unsigned char* dThresh = nb.thresh.as<unsigned char>();
    for (int s = 0, row = 0; s < 4; row += (int)W.anaOff[s].size(), ++s) {
        const int64_t n = (int64_t)W.anaOff[s].size();
        if (!n) continue;
        MRC_HIP(h, launch_nmr_source(h, pl.hs[s]->dev, n, dPlanes, (const int64_t*)(din + S.oAna[s]),
                                     (double*)(dLines + W.anaBytes[s]), nb.oscale.as<int>() + row,
                                     nb.smr.as<double>() + (int64_t)row * kMaxBands, (double*)(dThresh + W.anaBytes[s]), st));
    }
    MRC_HIP(h, hipEventRecord(nb.ev[3], st));
    unsigned char* dOut = nb.out.as<unsigned char>();
    for (int s = 0; s < 4; ++s) {
        if (W.ent[s].empty()) continue;
        MRC_HIP(h, launch_nmr_band(pl.hs[s]->dev, (int64_t)W.ent[s].size(), (const NmrEntry*)(din + S.oEnt[s]),
                                   (const UnpackGroupDev*)(din + S.oGroups), (const double*)(dLines + W.anaBytes[s]),
                                   (const double*)(dThresh + W.anaBytes[s]), detail ? (double*)(dOut + S.oNoise) : nullptr,
                                   detail ? (double*)(dOut + S.oMask) : nullptr, nb.stat.as<double>(), st));
    }
    MRC_HIP(h, launch_nmr_file(c.n_files, (const long long*)(din + S.oEntryStart), (const int*)(din + S.oNch),
                               nb.stat.as<double>(), (double*)(dOut + S.oFiles), st));
    MRC_HIP(h, hipMemcpyAsync(nb.pinOut.p, dOut, S.outTotal, hipMemcpyDeviceToHost, st));
    MRC_HIP(h, hipEventRecord(nb.ev[4], st));
    MRC_HIP(h, hipStreamSynchronize(st));
    for (int i = 0; i < 4; ++i) MRC_HIP(h, nb.ev.elapsed(i, i + 1, &nb.ms[i]));
    return MRC_OK;
}

// Results: one walk over (file, block) forms the file's weight (the sum of b over its blocks and channels) and names the
// entries' shapes; the dB values come from the file sums on the host (nmr_file_values); the bands are copied as they are.
void nmr_results(const mrc_config& cfg, const NmrCall& c, const PacPlan& pl, const NmrStage& S, const unsigned char* pout) {
    for (int64_t f = 0; f < c.n_files; ++f) {
        const int nch = pl.files[(size_t)f].nch;
        int64_t weight = 0;
        for (int64_t i = 0; i < pl.nBlocks(f); ++i) {
            int a, b;
            shape_ab(cfg, pl.shape(f, i), &a, &b);
            weight += (int64_t)b * nch;
            for (int ch = 0; c.entry_shape && ch < nch; ++ch) {
                const int64_t e = c.entry_offset[f] + i * nch + ch;
                c.entry_shape[2 * e] = a;
                c.entry_shape[2 * e + 1] = b;
            }
        }
        const NmrFileValues v = nmr_file_values((const double*)(pout + S.oFiles) + 4 * f, weight);
        c.nmr_total_db[f] = v.nmr_total_db;
        c.nmr_max_db[f] = v.nmr_max_db;
        c.disturbed_blocks[f] = v.disturbed_blocks;
    }
    if (c.detail() && c.nEntries()) {
        copy_host(c.band_noise, pout + S.oNoise, S.bandBytes);
        copy_host(c.band_mask, pout + S.oMask, S.bandBytes);
    }
}

}  // namespace

extern "C" {

int mrc_pac_nmr(mrc_handle* h, int64_t n_files, const uint8_t* buf, const int64_t* file_offset, const int16_t* src,
                const int64_t* src_offset, const int64_t* src_stride, const int64_t* src_frames, double* nmr_max_db,
                double* nmr_total_db, int64_t* disturbed_blocks, int64_t* n_blocks, int64_t* entry_offset, int64_t entry_cap,
                int32_t* entry_shape, double* band_noise, double* band_mask) {
    if (!h) return MRC_ERR_INVALID;
    const NmrCall c{n_files, buf, file_offset, src, src_offset, src_stride, src_frames, nmr_max_db, nmr_total_db,
                    disturbed_blocks, n_blocks, entry_offset, entry_cap, entry_shape, band_noise, band_mask};
    PacPlan pl;
    MRC_TRY(nmr_refusals(h, c, &pl));
    if (n_files == 0) return MRC_OK;
    MRC_TRY(ensure_decode_consts(h));
    NmrBufs& nb = h->nmr;
    MRC_HIP(h, nb.ev.create());
    MRC_TRY(pac_plan_groups(h, kFn, &pl));
    const NmrPlanes planes = nmr_source_planes(c, pl, h->cfg.n_mdct_lines);
    const NmrStage stage = nmr_stage_layout(c, pl, planes);
    MRC_HIP(h, nb.pinIn.reserve(stage.inTotal));
    MRC_HIP(h, nb.in.reserve(stage.inTotal));
    MRC_HIP(h, nb.groups.reserve(std::max<size_t>(pl.gBytes, 256)));
    const NmrWork work = nmr_fill_stage(h, c, pl, planes, stage, (unsigned char*)nb.pinIn.p);
    MRC_TRY(nmr_device(h, c, pl, planes, work, stage));
    nmr_results(h->cfg, c, pl, stage, (const unsigned char*)nb.pinOut.p);
    return MRC_OK;
}

int mrc_get_nmr_ms(mrc_handle* h, double* ms) {
    if (!h || !ms) return MRC_ERR_INVALID;
    for (int i = 0; i < 4; ++i) ms[i] = h->nmr.ms[i];
    return MRC_OK;
}

}  // extern "C"
