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

}  // namespace

extern "C" {

int mrc_pac_nmr(mrc_handle* h, int64_t n_files, const uint8_t* buf, const int64_t* file_offset, const int16_t* src,
                const int64_t* src_offset, const int64_t* src_stride, const int64_t* src_frames, double* nmr_max_db,
                double* nmr_total_db, int64_t* disturbed_blocks, int64_t* n_blocks, int64_t* entry_offset, int64_t entry_cap,
                int32_t* entry_shape, double* band_noise, double* band_mask) {
    if (!h) return MRC_ERR_INVALID;
    if (n_files < 0 || !file_offset || !src_offset || !src_stride || !src_frames || !nmr_max_db || !nmr_total_db ||
        !disturbed_blocks || !n_blocks || !entry_offset || entry_cap < 0 || (n_files > 0 && !buf) ||
        ((band_noise == nullptr) != (band_mask == nullptr)))
        return fail(h, MRC_ERR_INVALID, "mrc_pac_nmr: bad argument (band_noise and band_mask go together)");
    const int L = h->cfg.n_mdct_lines;
    const UnpackParams P = unpack_params(h->cfg);
    char msg[200];
    entry_offset[0] = 0;
    for (int64_t f = 0; f < n_files; ++f) {
        if (file_offset[0] < 0 || file_offset[f + 1] < file_offset[f])
            return fail(h, MRC_ERR_INVALID, "mrc_pac_nmr: file_offset must not decrease");
        if (src_offset[f] < 0 || src_stride[f] < 0 || src_frames[f] < 0 || (src_frames[f] > 0 && !src)) {
            std::snprintf(msg, sizeof msg, "mrc_pac_nmr: file %lld: negative source offset, stride or frame count, or no source",
                          (long long)f);
            return fail(h, MRC_ERR_INVALID, msg);
        }
    }
    if (n_files == 0) return MRC_OK;

    // ---- host plan (decode's; host only), entries, the NOMEM check before any device work
    const uint8_t* base = buf + file_offset[0];
    const int64_t inBytes = file_offset[n_files] - file_offset[0];
    PacPlan pl;
    MRC_TRY(pac_plan_scan(h, "mrc_pac_nmr", n_files, buf, file_offset, &pl));
    for (int64_t f = 0; f < n_files; ++f) {
        const PacFilePlan& fi = pl.files[(size_t)f];
        if (fi.nch == 2 && src_stride[f] < src_frames[f]) {
            std::snprintf(msg, sizeof msg, "mrc_pac_nmr: file %lld is stereo and its source stride %lld is below its %lld frames",
                          (long long)f, (long long)src_stride[f], (long long)src_frames[f]);
            return fail(h, MRC_ERR_INVALID, msg);
        }
        n_blocks[f] = pl.nBlocks(f);
        entry_offset[f + 1] = entry_offset[f] + fi.nChunks;     // one entry per (block, channel) = per chunk
    }
    const int64_t nEntries = entry_offset[n_files];
    const bool detail = band_noise != nullptr;
    if ((detail || entry_shape) && nEntries > entry_cap) {
        std::snprintf(msg, sizeof msg, "mrc_pac_nmr: the files hold %lld entries, entry_cap is %lld", (long long)nEntries,
                      (long long)entry_cap);
        return fail(h, MRC_ERR_NOMEM, msg);
    }
    MRC_TRY(ensure_decode_consts(h));
    DecodeBufs& d = h->dec;
    NmrBufs& nb = h->nmr;
    MRC_HIP(h, nb.ev.create());
    MRC_TRY(pac_plan_groups(h, "mrc_pac_nmr", &pl));
    const int64_t nChunks = pl.nChunks();

    // ---- source planes: one per distinct (first sample, frame count), as long as the longest file that reads it
    std::unordered_map<PlaneKey, int64_t, PlaneHash> planeOf;
    std::vector<NmrPlane> planes;
    std::vector<const int16_t*> planeSrc;
    std::vector<int64_t> fileChPlane((size_t)n_files * 2, -1);
    for (int64_t f = 0; f < n_files; ++f) {
        const PacFilePlan& fi = pl.files[(size_t)f];
        for (int c = 0; c < fi.nch; ++c) {
            const int16_t* p0 = src ? src + src_offset[f] + c * src_stride[f] : nullptr;
            const PlaneKey key{(uintptr_t)p0, src_frames[f]};
            auto it = planeOf.find(key);
            if (it == planeOf.end()) {
                it = planeOf.emplace(key, (int64_t)planes.size()).first;
                planes.push_back(NmrPlane{0, 0, src_frames[f], 0});
                planeSrc.push_back(p0);
            }
            NmrPlane& q = planes[(size_t)it->second];
            q.len = std::max<long long>(q.len, fi.extent);
            fileChPlane[(size_t)(2 * f + c)] = it->second;
        }
    }
    int64_t planeTotal = 0, srcTotal = 0, maxLen = 0;
    for (NmrPlane& q : planes) {
        q.frames = std::min<long long>(q.frames, std::max<long long>(0, q.len - L));   // samples a block reads
        q.dst = planeTotal;
        q.src = srcTotal;
        planeTotal += (q.len + 63) & ~63LL;
        srcTotal += q.frames;
        maxLen = std::max<int64_t>(maxLen, q.len);
    }

    // ---- entries and the distinct analyses, per block shape
    std::vector<NmrEntry> ent[4];
    std::vector<long long> anaOff[4];
    std::unordered_map<AnaKey, int64_t, AnaHash> anaOf;
    anaOf.reserve((size_t)nEntries);
    auto add_entry = [&](int64_t f, int64_t i, int g, int slot, int ch, int64_t start) {
        const int s = g / 2;
        int a, b;
        shape_ab(h->cfg, s, &a, &b);
        const int64_t plane = fileChPlane[(size_t)(2 * f + ch)];
        auto it = anaOf.find(AnaKey{plane, start, s});
        if (it == anaOf.end()) {
            it = anaOf.emplace(AnaKey{plane, start, s}, (int64_t)anaOff[s].size()).first;
            anaOff[s].push_back(planes[(size_t)plane].dst + start);
        }
        const int64_t e = entry_offset[f] + i * pl.files[(size_t)f].nch + ch;
        ent[s].push_back(NmrEntry{e, it->second, g, slot, ch, b});
    };

    // staging layout (one H2D copy): bytes | plan | groups | entries [4 shapes] | analysis offsets [4 shapes] |
    // entryStart [n+1] | nch [n] | planes | source samples
    size_t oEnt[4], oAna[4];
    const size_t oPlan = align256((size_t)inBytes), oGroups = oPlan + align256(sizeof(UnpackPlanEntry) * nChunks);
    size_t o = oGroups + align256(sizeof(UnpackGroupDev) * kUnpackGroups);
    // (entries per shape are known from the group slot counts: a joint slot is two entries, a non-joint slot one)
    for (int s = 0; s < 4; ++s) {
        oEnt[s] = o;
        o += align256(sizeof(NmrEntry) * (size_t)(2 * pl.nSlots[2 * s] + pl.nSlots[2 * s + 1]));
    }
    for (int s = 0; s < 4; ++s) {
        oAna[s] = o;
        o += align256(sizeof(long long) * (size_t)(2 * pl.nSlots[2 * s] + pl.nSlots[2 * s + 1]));
    }
    const size_t oEntryStart = o, oNch = oEntryStart + align256(sizeof(long long) * (n_files + 1)),
                 oPlanes = oNch + align256(sizeof(int) * n_files), oSrc = oPlanes + align256(sizeof(NmrPlane) * planes.size()),
                 inTotal = oSrc + align256(sizeof(int16_t) * (size_t)srcTotal);
    MRC_HIP(h, nb.pinIn.reserve(inTotal));
    MRC_HIP(h, nb.in.reserve(inTotal));
    MRC_HIP(h, nb.groups.reserve(std::max<size_t>(pl.gBytes, 256)));
    unsigned char* pin = (unsigned char*)nb.pinIn.p;
    copy_host(pin, base, (size_t)inBytes);
    pac_plan_fill(h->cfg, d, pl, (UnpackPlanEntry*)(pin + oPlan), (UnpackGroupDev*)(pin + oGroups), nb.groups.as<unsigned char>(),
                  [&](int64_t f, int64_t i, int g, int slot, int ch, int64_t start) {
                      if (g & 1) add_entry(f, i, g, slot, ch, start);                 // non-joint: one chunk, one entry
                      else { add_entry(f, i, g, slot, 0, start); add_entry(f, i, g, slot, 1, start); }
                  });
    size_t anaBytes[4], anaTotal = 0, anaRows = 0;
    for (int s = 0; s < 4; ++s) {
        std::memcpy(pin + oEnt[s], ent[s].data(), sizeof(NmrEntry) * ent[s].size());
        std::memcpy(pin + oAna[s], anaOff[s].data(), sizeof(long long) * anaOff[s].size());
        anaBytes[s] = anaTotal;
        anaTotal += align256(sizeof(double) * anaOff[s].size() * (size_t)d.bands.halfN[s]);
        anaRows += anaOff[s].size();
    }
    long long* entryStart = (long long*)(pin + oEntryStart);
    int* nchDev = (int*)(pin + oNch);
    for (int64_t f = 0; f <= n_files; ++f) entryStart[f] = entry_offset[f];
    for (int64_t f = 0; f < n_files; ++f) nchDev[f] = pl.files[(size_t)f].nch;
    std::memcpy(pin + oPlanes, planes.data(), sizeof(NmrPlane) * planes.size());
    for (size_t q = 0; q < planes.size(); ++q)
        if (planes[q].frames) copy_host(pin + oSrc + sizeof(int16_t) * planes[q].src, planeSrc[q], sizeof(int16_t) * planes[q].frames);

    // device buffers
    const size_t oNoise = align256(sizeof(double) * 4 * n_files), bandBytes = sizeof(double) * kMaxBands * (size_t)nEntries,
                 oMask = oNoise + align256(bandBytes), outTotal = detail ? oMask + bandBytes : oNoise;
    MRC_HIP(h, nb.planes.reserve(std::max<size_t>(sizeof(int16_t) * planeTotal, 256)));
    MRC_HIP(h, nb.lines.reserve(std::max<size_t>(anaTotal, 256)));
    MRC_HIP(h, nb.thresh.reserve(std::max<size_t>(anaTotal, 256)));
    MRC_HIP(h, nb.oscale.reserve(std::max<size_t>(sizeof(int) * anaRows, 256)));
    MRC_HIP(h, nb.smr.reserve(std::max<size_t>(sizeof(double) * kMaxBands * anaRows, 256)));
    MRC_HIP(h, nb.stat.reserve(std::max<size_t>(sizeof(double) * 2 * nEntries, 256)));
    MRC_HIP(h, nb.out.reserve(outTotal));
    MRC_HIP(h, nb.pinOut.reserve(outTotal));

    // ---- device
    hipStream_t st = h->stream;
    unsigned char* din = nb.in.as<unsigned char>();
    MRC_HIP(h, hipEventRecord(nb.ev[0], st));
    MRC_HIP(h, hipMemcpyAsync(din, pin, inTotal, hipMemcpyHostToDevice, st));
    MRC_HIP(h, hipEventRecord(nb.ev[1], st));
    MRC_TRY(reset_unpack_err(h, st));
    MRC_HIP(h, launch_unpack_dense(P, d.bands, d.consts.as<UnpackTables>(), nChunks, (const UnpackPlanEntry*)(din + oPlan),
                                   din, inBytes, (const UnpackGroupDev*)(din + oGroups), d.err.as<UnpackErr>(), st));
    MRC_HIP(h, hipEventRecord(nb.ev[2], st));
    MRC_HIP(h, hipMemcpyAsync(d.pinErr.get(), d.err.p, sizeof(UnpackErr), hipMemcpyDeviceToHost, st));
    MRC_HIP(h, hipStreamSynchronize(st));
    if (d.pinErr->flag) {
        const UnpackPlanEntry* plan = (const UnpackPlanEntry*)(pin + oPlan);
        const int64_t c = d.pinErr->firstBad;
        const int64_t at = c < nChunks ? plan[c].off + file_offset[0] : 0;
        const int64_t f = std::upper_bound(file_offset, file_offset + n_files + 1, at) - file_offset - 1;
        std::snprintf(msg, sizeof msg, "mrc_pac_nmr: file %lld: chunk at byte %lld: %s", (long long)f,
                      (long long)(at - file_offset[std::max<int64_t>(f, 0)]), unpack_status_text(d.pinErr->flag));
        return fail(h, MRC_ERR_INVALID, msg);
    }
    short* dPlanes = nb.planes.as<short>();
    MRC_HIP(h, launch_nmr_pad((int64_t)planes.size(), (const NmrPlane*)(din + oPlanes), maxLen, L,
                              (const short*)(din + oSrc), dPlanes, st));
    unsigned char* dLines = nb.lines.as<unsigned char>();
    unsigned char* dThresh = nb.thresh.as<unsigned char>();
    for (int s = 0, row = 0; s < 4; row += (int)anaOff[s].size(), ++s) {
        const int64_t n = (int64_t)anaOff[s].size();
        if (!n) continue;
        const DevShape& S = pl.hs[s]->dev;
        double* X = (double*)(dLines + anaBytes[s]);
        double* T = (double*)(dThresh + anaBytes[s]);
        int* os = nb.oscale.as<int>() + row;
        const int64_t* offs = (const int64_t*)(din + oAna[s]);
        MRC_HIP(h, launch_nmr_source(h, S, n, dPlanes, offs, X, os, nb.smr.as<double>() + (int64_t)row * kMaxBands, T, st));
    }
    MRC_HIP(h, hipEventRecord(nb.ev[3], st));
    unsigned char* dOut = nb.out.as<unsigned char>();
    for (int s = 0; s < 4; ++s) {
        if (ent[s].empty()) continue;
        MRC_HIP(h, launch_nmr_band(pl.hs[s]->dev, (int64_t)ent[s].size(), (const NmrEntry*)(din + oEnt[s]),
                                   (const UnpackGroupDev*)(din + oGroups), (const double*)(dLines + anaBytes[s]),
                                   (const double*)(dThresh + anaBytes[s]), detail ? (double*)(dOut + oNoise) : nullptr,
                                   detail ? (double*)(dOut + oMask) : nullptr, nb.stat.as<double>(), st));
    }
    MRC_HIP(h, launch_nmr_file(n_files, (const long long*)(din + oEntryStart), (const int*)(din + oNch), nb.stat.as<double>(),
                               (double*)dOut, st));
    MRC_HIP(h, hipMemcpyAsync(nb.pinOut.p, dOut, outTotal, hipMemcpyDeviceToHost, st));
    MRC_HIP(h, hipEventRecord(nb.ev[4], st));
    MRC_HIP(h, hipStreamSynchronize(st));
    for (int i = 0; i < 4; ++i) MRC_HIP(h, nb.ev.elapsed(i, i + 1, &nb.ms[i]));

    // ---- results: dB on the host from the file sums
    const unsigned char* pout = (const unsigned char*)nb.pinOut.p;
    const double* fileOut = (const double*)pout;
    for (int64_t f = 0; f < n_files; ++f) {
        const PacFilePlan& fi = pl.files[(size_t)f];
        int64_t weight = 0;
        for (int64_t i = 0; i < pl.nBlocks(f); ++i) {
            int a, b;
            shape_ab(h->cfg, pl.shape(f, i), &a, &b);
            weight += (int64_t)b * fi.nch;
        }
        const NmrFileValues v = nmr_file_values(fileOut + 4 * f, weight);
        nmr_total_db[f] = v.nmr_total_db;
        nmr_max_db[f] = v.nmr_max_db;
        disturbed_blocks[f] = v.disturbed_blocks;
    }
    if (entry_shape)
        for (int64_t f = 0; f < n_files; ++f)
            for (int64_t i = 0; i < pl.nBlocks(f); ++i)
                for (int c = 0; c < pl.files[(size_t)f].nch; ++c) {
                    int a, b;
                    shape_ab(h->cfg, pl.shape(f, i), &a, &b);
                    const int64_t e = entry_offset[f] + i * pl.files[(size_t)f].nch + c;
                    entry_shape[2 * e] = a;
                    entry_shape[2 * e + 1] = b;
                }
    if (detail && nEntries) {
        copy_host(band_noise, pout + oNoise, bandBytes);
        copy_host(band_mask, pout + oMask, bandBytes);
    }
    return MRC_OK;
}

int mrc_get_nmr_ms(mrc_handle* h, double* ms) {
    if (!h || !ms) return MRC_ERR_INVALID;
    for (int i = 0; i < 4; ++i) ms[i] = h->nmr.ms[i];
    return MRC_OK;
}

}  // extern "C"
