// C ABI, resident `.pac` store (include/mrc_hip.h: mrc_pac_store_*): files uploaded once, sample windows decoded into the
// caller's device memory.
//
// create: pac_plan_scan -- the host plan of mrc_decode_pac_pcm16, one scan in the tree -- gives every file's chunks, block
// shapes and positions; the bytes go to the device in one copy and never cross PCIe again.
//
// The window calls (decode_window and its nine kin, stft_window and stft_window_routed) are one path:
//   request   every extern "C" entry fills a WindowRequest -- what the widest entry takes, the caller's arrays as they came --
//             and does nothing else.
//   check     check_windows turns it into a CheckedWindows once per public call: the internal mix, the one filter or the list
//             of them, the line-to-band tables, the term count, the longest pre-roll.  Every refusal of every entry is there,
//             in the order the entry gives them; no loop checks an argument again.
//   loops     units_loop decodes units (items or terms) into rows; reverb_loop has it decode a slab's terms dry and convolves
//             and folds them; stft_loop has reverb_loop make a slab's rows and transforms them.  Each takes the checked
//             request and a WindowRun: a row range, the window, format and output of that range, and the slab limit -- 0 when
//             the caller has cut the slab itself.  An outer loop hands the inner one a range; the arrays are indexed by the
//             call's own row and term numbers throughout and no temporary ones are built.
//   totals    the store's stats, ms, reverbMs and stftMs are the accumulator: the entry zeroes them, the slabs add to them.
// block_energy, band_energy_window and filterbank_window are families of their own over the same slab plan (stage_slab,
// parse_slab); the mix check, the file check, the elapsed-time sums and the copy of the energy entries have one definition
// for all three families.
//
// units_loop, per slab of whole rows (an item call's row is its one unit):
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
// dequantises the first 1 / D of a block's lines and runs the inverse transform of the shape (a, b) / D.  The one loop holds
// the arithmetic for every D.
//
// decode_window_mix, one channel of every item (left, right or the mid (L + R) / 2): the same plan with ONE plane per item
// and one workgroup per needed block (decode_mix_kernel, its selector an argument).  A joint block keeps its slot of two
// chunks -- the M/S switches and both streams are needed even for left.  The non-joint last block of a stereo file is one
// single slot for left / right (the other channel's chunk is not in the plan) and for mid a PAIR: two neighbouring slots
// of the non-joint group, which laid side by side are one slot of two streams, the group's pairs in front of its single
// slots so that a workgroup finds its slot from its index alone.  pac_plan_layout sees slot counts as ever.
//
// decode_window_resampled, the windows at up / down of the rate 1 / D: the units loop with two coordinate systems.  start and
// window count output samples; what is planned, staged, parsed and synthesised is each item's span of INTERMEDIATE samples
// (everything the filter reads for the item's outputs), and resample_out_kernel folds the planes into the caller's tensor
// where window_out_kernel copies them.  The filter (mrc_resample_taps.hpp: host only) goes up once per handle and
// (up, down, zeros, rolloff).
//
// decode_window_sum, rows that are weighted sums of windows: the units loop with the TERM as its planning unit.  Each term is
// planned, staged, parsed and synthesised as an item of the calls above, into planes of its own; a slab is a run of whole
// rows counted by its terms' spans, and sum_out_kernel / resample_sum_out_kernel fold a row's terms with their gains, in the
// order given, into the caller's tensor.  The term records (WindowItem, gain, output start) and the rows' term offsets go up
// with the plan.  No per-term window is written.
//
// decode_window_shaped, those rows with a band gain on every decoded MDCT line: the units loop with a shaping spec beside the
// filter and the rows.  Per call one uint16 line-to-band table per block shape (band_line_ranges over the FULL shape, at every
// D); per slab, in the same staging copy as the plan, those tables, the slab's rows of gains and one unit index per slot or
// workgroup laid out as the block offsets are; the shaped launches (mrc_kernels_decode.hip) multiply once per line between
// the dequantiser and the inverse transform.  Calls without gains never come here.
//
// decode_window_speeds, those rows with a ratio per term: the units loop with a list of filters beside the rows.  Each term's
// span is its own ratio's; the planes have one length per call, the largest span among the ratios named plus 4 L, so the
// synthesis launches and their second plane at x + planeLen stay as they are.  The terms' ratio indices and the table of
// the ratios (SpeedRatio) ride in the slab's staging copy; SumTerm and WindowItem are the other calls', unchanged.
//
// decode_window_reverb, those rows with a room impulse response per term: NOT another spec of the units loop but a loop of
// its own (reverb_loop), which has the units loop decode every term of a slab, as a row of its own, over its span lengthened
// by the pre-roll into a float64 scratch buffer; reverb_forward_kernel and reverb_fold_kernel (mrc_kernels_reverb.hip:
// partitioned overlap-save) then make the rows.  The bank's partition spectra live in the store (set_irs), made once by the
// same forward kernel.
//
// stft_window, the short-time Fourier transform of those rows: stft_loop has reverb_loop write a slab's rows as float64 into
// a second scratch buffer and stft_kernel (mrc_kernels_stft.hip) frames and transforms them.
//
// decode_window_routed and stft_window_routed, rows of several OUTPUT channels with a gain and a response per (term, channel):
// the routed kinds of the request, through the same reverb_loop.  A term is decoded with one channel, once; its routes stand
// where the reverb call has one gain and one response; it gets a source of forward transforms per distinct response length
// among its wet routes, and reverb_route_fold_kernel writes the rows' channels.  The STFT loop sees rows of that many channels.
//
// decode_window_spans and stft_window_spans, terms that sound in part of their row and fade at its ends: the reverb and STFT
// requests with four more arrays, and no loop of their own.  The units loop narrows what it plans for a term to the term's span cut
// to the row (under termRows moved up by the pre-roll), sizes the planes by the longest span of the range instead of the window,
// sends a TermSpan record per term up beside the SumTerms and launches the span kernels (mrc_kernels_store_span.hip); reverb_loop
// and stft_loop read their terms through it as ever.  A request without spans runs what it ran.
//
// block_energy, ((a + b) / D) * the sum of squares of a block's first 1 / D decoded lines, per channel or for the mid, for
// every block of the selected files: the same slab plan (stage_slab, parse_slab) over runs of whole blocks instead of the
// blocks of windows, then block_energy_kernel per group (mrc_kernels_store.hip) in place of planes, synthesis and output.
//
// band_energy_window, those sums split by frequency band and laid on a frame grid: the same slab plan over the blocks whose
// TILE [p + a / 2 - L, p + a + b / 2 - L) the item's frames overlap (tiles abut, so the needed blocks are one run found by two
// binary searches in the file's edges, kept doubled so that half samples are integers), band_energy_kernel per group into
// B [row][band] of the store workspace -- a row per needed block and decoded channel, an item's rows together -- then
// band_frames_kernel over the slab's output; per item one descriptor and its run of edges go up with the plan, per shape
// the band's line ranges (mrc_band_line_ranges, no handle and no device).
//
// filterbank_window, the same call with a bank of triangular filters in place of the rectangular bands: one body
// (energy_frames_window) serves both, and what differs is an EnergyTable -- the words that go up per slab beside the items
// and edges, and the launcher called per group.  The filter call's table is, per shape, lo, hi and a row offset per filter
// and the rows of mrc_filterbank_line_weights (host float64, no handle and no device), computed once per call.
#include "mrc_handle.hpp"
#include "mrc_resample_taps.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>

using namespace mrc;

namespace {

const char* const kWin = "mrc_pac_store_decode_window";
const char* const kWinReduced = "mrc_pac_store_decode_window_reduced";
const char* const kWinMix = "mrc_pac_store_decode_window_mix";
const char* const kWinResampled = "mrc_pac_store_decode_window_resampled";
const char* const kWinSum = "mrc_pac_store_decode_window_sum";
const char* const kWinShaped = "mrc_pac_store_decode_window_shaped";
const char* const kWinSpeeds = "mrc_pac_store_decode_window_speeds";
constexpr int kNoMix = -1;                           // the internal mix: every channel of a file into a plane of its own

int store_alive(mrc_pac_store* s, const char* fn) {
    if (!s) return fail(nullptr, MRC_ERR_INVALID, std::string(fn) + ": null store");
    if (!s->h) return fail(nullptr, MRC_ERR_INVALID, std::string(fn) + ": the store's handle has been destroyed");
    return MRC_OK;
}

using Need = StoreNeed;                              // (item: index in the slab)

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

// rate_divisor of every call that takes one: 1, 2 or 4, and a reduced shape for each of the handle's four block shapes
int check_divisor(mrc_handle* h, const std::string& w, int D) {
    if (D != 1 && D != 2 && D != 4) return fail(h, MRC_ERR_INVALID, w + ": rate_divisor " + std::to_string(D) + " is not 1, 2 or 4");
    for (int sh = 0; D > 1 && sh < 4; ++sh) {
        int a, b;
        shape_ab(h->cfg, sh, &a, &b);
        const std::string refusal = synth_shape_refusal(a, b, D);
        if (!refusal.empty()) return fail(h, MRC_ERR_INVALID, w + ": " + refusal);
    }
    return MRC_OK;
}

// mix of every call that takes one: a member of `allowed`, a set of bits 1 << MRC_MIX_*; the refusal names the set
constexpr unsigned kMixEachOrMid = 1u << MRC_MIX_EACH | 1u << MRC_MIX_MID, kMixOfOne = 1u << MRC_MIX_MID | 1u << MRC_MIX_LEFT | 1u << MRC_MIX_RIGHT,
                   kMixAny = kMixOfOne | 1u << MRC_MIX_EACH;
int check_mix(mrc_handle* h, const std::string& w, int mix, unsigned allowed) {
    if (mix >= 0 && mix < 4 && (allowed >> mix & 1)) return MRC_OK;
    const struct { int v; const char* name; } all[4] = {{MRC_MIX_EACH, "MRC_MIX_EACH (3)"}, {MRC_MIX_MID, "MRC_MIX_MID (0)"},
                                                       {MRC_MIX_LEFT, "MRC_MIX_LEFT (1)"}, {MRC_MIX_RIGHT, "MRC_MIX_RIGHT (2)"}};
    std::string names;
    for (int i = 0, left = __builtin_popcount(allowed); i < 4; ++i)
        if (allowed >> all[i].v & 1) names += std::string(all[i].name) + (--left > 1 ? ", " : left == 1 ? " or " : "");
    return fail(h, MRC_ERR_INVALID, w + ": mix " + std::to_string(mix) + " is not " + names);
}

// file[k] (null: k itself) of every k < n is a file of the store, and -- maxChannels 1 or 2; 0: not looked at -- has no more
// channels than that; `unit` is what k counts in the second refusal ("item", "term")
int check_files(mrc_pac_store* s, const std::string& w, int64_t n, const int64_t* file, int maxChannels, const char* unit) {
    const int64_t nFiles = (int64_t)s->index.files.size();
    for (int64_t k = 0; k < n; ++k) {
        const int64_t f = file ? file[k] : k;
        if (f < 0 || f >= nFiles)
            return fail(s->h, MRC_ERR_INVALID, w + ": file[" + std::to_string(k) + "] = " + std::to_string(f) + " is outside the store's " +
                                                   std::to_string(nFiles) + " files");
        if (maxChannels && s->index.files[(size_t)f].nch > maxChannels)
            return fail(s->h, MRC_ERR_INVALID, w + ": " + unit + " " + std::to_string(k) + ": file " + std::to_string(f) +
                                                   " is stereo, the call asks for one channel");
    }
    return MRC_OK;
}

// The statistics of a call are kept in the store itself: the entry point zeroes them, every slab of every loop adds to them
// (stage_slab its chunks and bytes), and nothing is saved, summed or restored on the way.
void reset_stats(mrc_pac_store* s) {
    for (int i = 0; i < 4; ++i) { s->stats[i] = 0; s->ms[i] = 0.0; }
}
// ms[i] += the time between events pair[i][0] and pair[i][1] of a slab that has been synchronised
constexpr int kSlabSpans[4][2] = {{0, 1}, {1, 2}, {3, 4}, {4, 5}};      // StoreBufs::ev: upload | unpack | synthesis | output
template <class Events>
int add_elapsed(mrc_handle* h, const Events& ev, const int (*pair)[2], int n, double* ms) {
    for (int i = 0; i < n; ++i) {
        double t = 0.0;
        MRC_HIP(h, ev.elapsed(pair[i][0], pair[i][1], &t));
        ms[i] += t;
    }
    return MRC_OK;
}

// The host side of one slab's parse, shared by units_loop, block_energy and energy_frames_window: `needs`, the slab's blocks,
// become slots of the (shape, kind) groups and plan entries that point into the resident bytes.
//   slots    a joint block is one slot of two streams.  Any other block is one slot per chunk parsed: all of the file's, or
//            under MRC_MIX_LEFT / _RIGHT the one asked for.  Under MRC_MIX_MID the two chunks of a stereo file's last block
//            are a PAIR of neighbouring slots, the group's pairs in front of its single slots (nPairs per group).
//   staging  plan | group descriptors | whatever more(&lay) adds once the slots are counted (pl holds them);
//            StoreBufs' pinIn, in and groups are reserved for it, the descriptors and the plan entries written.
//   visit(need, g, slot, ch, pair)   once per joint block (ch 0) and once per parsed chunk of any other block, in the
//            order of `needs`: the caller's per-slot fields (pin is valid by then).
// Counts the chunks and the staging's bytes into the store's stats.  What follows is pac_parse over the same fields.
struct SlabStage {
    size_t oPlan = 0, oGroups = 0, total = 0;
    int64_t nChunks = 0, nPairs[kUnpackGroups] = {};
    unsigned char* pin = nullptr;
    UnpackGroupDev* gd = nullptr;                    // (in pin)
};
template <class More, class Visit>
int stage_slab(mrc_pac_store* s, const char* fn, int mix, const std::vector<Need>& needs, PacPlan* plp, SlabStage* S, More more,
               Visit visit) {
    mrc_handle* h = s->h;
    StoreBufs& b = h->store;
    PacPlan& pl = *plp;
    // chunks of a needed non-joint block that are parsed
    const auto lastChunks = [mix](int nch) { return mix == MRC_MIX_LEFT || mix == MRC_MIX_RIGHT ? 1 : nch; };
    pl.clear_counts();
    *S = SlabStage{};
    for (const Need& n : needs) {
        const int nch = lastChunks(s->index.files[(size_t)n.file].nch), sh = s->index.shape(n.file, n.block);
        const bool joint = n.block < s->index.nJoint(n.file);
        pl.add_block(sh, joint, nch);
        if (!joint && mix == MRC_MIX_MID && nch == 2) S->nPairs[sh * 2 + 1] += 1;
    }
    MRC_TRY(pac_plan_layout(h, fn, &pl));
    S->nChunks = pl.nEntries();

    StageLayout lay(256);
    S->oPlan = lay.add<UnpackPlanEntry>(S->nChunks);
    S->oGroups = lay.add<UnpackGroupDev>(kUnpackGroups);
    more(&lay);
    S->total = lay.total();
    MRC_HIP(h, b.pinIn.reserve(S->total));
    MRC_HIP(h, b.in.reserve(S->total));
    MRC_HIP(h, b.groups.reserve(std::max<size_t>(pl.gBytes, 256)));
    S->pin = (unsigned char*)b.pinIn.p;
    S->gd = (UnpackGroupDev*)(S->pin + S->oGroups);
    UnpackPlanEntry* plan = (UnpackPlanEntry*)(S->pin + S->oPlan);
    pac_plan_group_descs(h->dec, pl, S->gd, b.groups.as<unsigned char>());
    int64_t catPos[2 * kUnpackGroups], slotNext[kUnpackGroups] = {}, pairNext[kUnpackGroups] = {};
    for (int64_t k = 0, q = 0; k < 2 * kUnpackGroups; q += pl.nCat[k], ++k) catPos[k] = q;
    for (int g = 0; g < kUnpackGroups; ++g) slotNext[g] = 2 * S->nPairs[g];      // (joint groups, and every group without mid: 0)
    for (const Need& n : needs) {
        const PacFilePlan& fi = s->index.files[(size_t)n.file];
        const int64_t c0 = fi.firstChunk + n.block * fi.nch;
        const int sh = s->index.chunkShape[(size_t)c0];
        if (n.block < s->index.nJoint(n.file)) {
            const int g = sh * 2, slot = (int)slotNext[g]++;
            for (int ch = 0; ch < 2; ++ch)
                plan[catPos[sh * 4 + ch]++] = UnpackPlanEntry{s->index.chunkOff[(size_t)c0 + ch], g * 2 + ch, slot};
            visit(n, g, slot, 0, false);
        } else {
            const int g = sh * 2 + 1, nParsed = lastChunks(fi.nch), ch0 = fi.nch == 2 && mix == MRC_MIX_RIGHT ? 1 : 0;
            const bool pair = mix == MRC_MIX_MID && fi.nch == 2;
            for (int ch = ch0; ch < ch0 + nParsed; ++ch) {
                const int slot = (int)(pair ? pairNext[g]++ : slotNext[g]++);
                plan[catPos[sh * 4 + 2]++] = UnpackPlanEntry{s->index.chunkOff[(size_t)c0 + ch], g * 2, slot};
                visit(n, g, slot, ch, pair);
            }
        }
    }
    s->stats[0] += S->nChunks;
    s->stats[3] += (int64_t)S->total;
    return MRC_OK;
}
// ... and its device side: the staging to the device, unpack_dense_kernel over the plan, the parser's verdict (pac_parse)
int parse_slab(mrc_pac_store* s, const char* fn, const SlabStage& S, hipStream_t st) {
    StoreBufs& b = s->h->store;
    return pac_parse(s->h, fn, s->index.fileBase,
                     PacParse{S.pin, b.in.p, S.total, S.oPlan, S.oGroups, S.nChunks, s->bytes.as<uint8_t>(), s->nBytes,
                              {b.ev[0], b.ev[1], b.ev[2]}, st});
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
        int64_t start = 0, tileEnd = 0;
        for (int64_t i = 0; i < s->index.nBlocks(f); ++i) {
            int a, b;
            shape_ab(h->cfg, s->index.shape(f, i), &a, &b);
            s->blockStart.push_back(start);
            s->tileEdge.push_back(2 * start + a - 2 * (int64_t)h->cfg.n_mdct_lines);
            tileEnd = 2 * start + 2 * a + b - 2 * (int64_t)h->cfg.n_mdct_lines;
            start += a;
        }
        s->tileEdge.push_back(tileEnd);                      // (a file's edges: its blocks' + 1, from firstBlock[f] + f on)
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

int64_t floor_div(int64_t a, int64_t b) {             // b > 0
    const int64_t q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// the device table of a filter, computed and uploaded on its first use on this handle
int get_resample_table(mrc_handle* h, const ResampleSpec& r, const ResampleTable** out) {
    auto& tables = h->store.resample;
    const auto key = std::make_tuple(r.up, r.down, r.zeros, r.rolloff);
    auto it = tables.find(key);
    if (it == tables.end()) {
        if (tables.size() >= 16) tables.clear();             // (a sweep over ratios: no call is in flight between calls)
        const size_t nTaps = 2 * (size_t)r.W, n = nTaps * (size_t)r.up;
        std::vector<double> byPhase(n), byTap(n);
        resample_taps(r, byPhase.data());
        for (size_t p = 0; p < (size_t)r.up; ++p)
            for (size_t j = 0; j < nTaps; ++j) byTap[j * (size_t)r.up + p] = byPhase[p * nTaps + j];
        ResampleTable t;
        t.W = r.W;
        int g = 1;
        resample_lds_layout(r.up, r.down, &g, &t.skew);
        t.evenOdd = g == 2;
        t.skewNatural = resample_lds_cycles(r.up, r.down, 1, 1) < resample_lds_cycles(r.up, r.down, 1, 0);
        MRC_HIP(h, t.taps.reserve(sizeof(double) * n));
        MRC_HIP(h, hipMemcpy(t.taps.p, byTap.data(), sizeof(double) * n, hipMemcpyHostToDevice));
        it = tables.emplace(key, std::move(t)).first;
    }
    *out = &it->second;
    return MRC_OK;
}

// mrc_pac_store_decode_window_speeds: the tables of all the call's filters, none evicted while a later one is resolved -- the
// cache is emptied BEFORE the first when the missing ones would not fit beside what it holds (get_resample_table then never
// finds it full)
int get_resample_tables(mrc_handle* h, int n, const ResampleSpec* r, const ResampleTable** out) {
    auto& tables = h->store.resample;
    std::map<std::tuple<int, int, int, double>, int> missing;
    for (int i = 0; i < n; ++i) {
        const auto key = std::make_tuple(r[i].up, r[i].down, r[i].zeros, r[i].rolloff);
        if (r[i].W && tables.find(key) == tables.end()) missing[key] = 1;
    }
    if (tables.size() + missing.size() > 16) tables.clear();
    for (int i = 0; i < n; ++i) {
        out[i] = nullptr;
        if (r[i].W) MRC_TRY(get_resample_table(h, r[i], &out[i]));
    }
    return MRC_OK;
}

// ---- the window calls: one request, checked once, run by three loops over row ranges (see the head of the file)
// What the widest entry takes, without the STFT's own arguments.  Every extern "C" window entry fills one and nothing else.
struct WindowRequest {
    enum Kind { kItems, kRows, kReverb, kStft, kRouted, kStftRouted };   // which checks are made and in what order (check_windows)
    const char* fn;                                          // the entry point's name, in front of every refusal
    Kind kind;
    int rateDivisor = 1;
    int mix = MRC_MIX_EACH;                                  // the caller's MRC_MIX_*, one of mixAllowed
    unsigned mixAllowed = kMixAny;
    // the ratio: none, one (up, down) -- an item call's must differ from 1, a rows call's may be 1 -- or a list with ratioOf
    bool resampled = false;
    int up = 1, down = 1;
    bool ratioList = false;
    int nRatios = 0;
    const int32_t *ratioUp = nullptr, *ratioDown = nullptr, *ratioOf = nullptr;
    int zeros = 0;
    double rolloff = 0.0;
    bool banded = false;                                     // band gains on the MDCT lines (with a ratio list: n_bands != 0)
    int nBands = 0;
    const double *edgeHz = nullptr, *bandGain = nullptr;
    int64_t nItems = 0;                                      // rows; an item call's rows are its units
    const int64_t *termOffset = nullptr, *file = nullptr, *start = nullptr;
    const double* gain = nullptr;
    const int32_t* irOf = nullptr;
    // the audible span of every term in row samples and its linear fades (spanFirst NULL: every term is the whole row, the
    // call as it was; a NULL fade array: 0)
    const int64_t *spanFirst = nullptr, *spanLen = nullptr, *fadeIn = nullptr, *fadeOut = nullptr;
    int nChannelsOut = 1;                                    // the channels DECODED per unit and, unless routed, written per row
    // a routed kind: every term gives one channel (nChannelsOut == 1) and reaches routeChannels output channels; gain and irOf
    // are then the route arrays, [n_terms][routeChannels]
    int routeChannels = 0;
    void* stream = nullptr;
    bool rows() const { return kind != kItems; }
    bool spans() const { return spanFirst != nullptr; }
    bool routed() const { return kind == kRouted || kind == kStftRouted; }
    bool stft() const { return kind == kStft || kind == kStftRouted; }
    bool banked() const { return kind != kItems && kind != kRows; }
    int routesPerTerm() const { return routed() ? routeChannels : 1; }   // the stride of gain and irOf
    int rowChannels() const { return routed() ? routeChannels : nChannelsOut; }
};
struct SpeedSpec {
    int nRatios;
    ResampleSpec r[MRC_MAX_STORE_RATIOS];                    // reduced; W == 0: the unit ratio, no filter
};
struct ShapeSpec {
    std::vector<uint16_t> lineBand;                          // the band of every line of the four block shapes, shape after shape
    int64_t lineOff[4];                                      // ... shape sh from lineOff[sh] on, (a + b) / 2 values
};
// What check_windows makes of a request, once per public call: the arrays stay the request's, indexed by the call's own
// row and term numbers in every loop -- no loop re-bases them.
struct CheckedWindows {
    WindowRequest q;
    int mix = kNoMix;                                        // kNoMix or MRC_MIX_MID / _LEFT / _RIGHT
    int64_t nTerms = 0;                                      // the units: terms of a rows call, items of an item call
    bool filtered = false, speedy = false, shaped = false;   // which of the three specs below is in use
    ResampleSpec rs;                                         // one ratio other than 1 for every unit
    SpeedSpec speeds;                                        // a ratio per term (only where there are terms)
    ShapeSpec shape;
    int64_t maxPreRoll = 0;                                  // the longest response named by any term - 1
    bool empty = false;                                      // no row or no sample: nothing to launch
};
// What a loop is asked to run: rows [first, last) of the checked request into `out`, which is row first's.
struct WindowRun {
    int64_t first, last;
    int64_t window;
    int format;
    void* out;
    int64_t slab;                                            // the slab limit in samples; 0: the range is one slab (a caller cut it)
    int64_t preRoll = 0;                                     // units_loop: every start moved down by it, saturating at INT64_MIN
    bool termRows = false;                                   // units_loop: first and last count TERMS, each a row of its own at gain 1.0
};

// The units loop: D the rate divisor (1: full rate, decode_kernel), c.mix kNoMix or one channel of every unit (one plane per
// unit, decode_mix_kernel; n_channels_out is then 1).  What is planned, staged, parsed and synthesised is the UNIT,
// (file[k], start[k]): an item, or with rows a TERM of row i, k in [termOffset[i], termOffset[i + 1]).  A slab is a run of
// whole rows, counted by its units' spans; sum_out_kernel / resample_sum_out_kernel fold a row's terms with their gains
// where the item calls copy or fold one unit per row.
// c.filtered (one ratio): start and window count OUTPUT samples, at up / down of the rate 1 / D.  Unit k reads the
// intermediate samples [lo, hi], lo = floor(start down / up) - W + 1, hi = floor((start + window - 1) down / up) + W: that
// span is what is planned, staged, parsed and synthesised exactly as a window of the other calls -- into planes of span + 4 L
// samples, span = ceil((window - 1) down / up) + 2 W the one bound on hi - lo + 1 -- and resample_out_kernel stands where
// window_out_kernel stands.  A slab counts plane samples (spans).
// c.speedy (a ratio per term): term k is planned over the span of ITS ratio -- the unit ratio's is [start, start + window) --
// into planes of ONE length, the largest span bound among the ratios the range's terms name plus 4 L, which a slab counts
// each term at.  Per slab, in the one staging copy: the ratio index of every term and the table of the ratios (SpeedRatio);
// resample_multi_sum_out_kernel folds.
// c.shaped (band gains, one row per unit): each needed block is synthesised by the shaped launches, its line k multiplied
// once by the unit's gain of the band that band_line_ranges(sample rate, the block's FULL shape) puts it in, whatever D.  Per
// slab, in the one staging copy: the line-to-band tables, the slab's rows of gains, and one unit index per slot or workgroup
// laid out as the block offsets are.
// run.termRows and run.preRoll are the reverb loop's: the terms [first, last) as rows of one term each at gain 1.0, read
// from start - preRoll.  They go through the sum kernels with SumTerm records like any row: 0.0 + 1.0 * v is v, and a -0.0
// becomes +0.0, which no fold from +0.0 can tell apart.
int units_loop(mrc_pac_store* s, const CheckedWindows& c, const WindowRun& run) {
    const WindowRequest& q = c.q;
    mrc_handle* h = s->h;
    const mrc_config& cfg = h->cfg;
    const char* const fn = q.fn;
    const int D = q.rateDivisor, mix = c.mix, n_channels_out = q.nChannelsOut, format = run.format;
    const int64_t* const file = q.file;
    const int64_t window = run.window, L = cfg.n_mdct_lines / D;             // L: the margin unit, reduced samples
    const bool sum = q.rows();
    const ResampleSpec* const rs = c.filtered ? &c.rs : nullptr;
    const SpeedSpec* const speeds = c.speedy ? &c.speeds : nullptr;
    const ShapeSpec* const shape = c.shaped ? &c.shape : nullptr;
    const int64_t* const rowTerms = sum && !run.termRows ? q.termOffset : nullptr;
    const auto unitsBefore = [rowTerms](int64_t row) { return rowTerms ? rowTerms[row] : row; };
    // (a start that far down is below every file with or without the pre-roll)
    const auto startOf = [&](int64_t k) { return q.start[k] < INT64_MIN + run.preRoll ? INT64_MIN : q.start[k] - run.preRoll; };
    // spans: term k sounds at the run's row samples [a0, a1) = its span, moved up by the pre-roll as the run's rows begin that
    // much before the call's, cut to the row -> whether that is any sample.  Without spans every term is the whole row.
    const bool spans = q.spans();
    // (spans come with a list of ratios, the reverb and STFT entries' arguments: asked before anything is launched)
    if (spans && !q.ratioList) return fail(s->h, MRC_ERR_INVALID, std::string(q.fn) + ": internal error: spans without a list of ratios");
    const auto audible = [&](int64_t k, int64_t* a0, int64_t* a1) {
        *a0 = 0;
        *a1 = window;
        if (!spans) return true;
        const int64_t f = q.spanFirst[k] + run.preRoll;
        *a0 = std::max<int64_t>(f, 0);
        *a1 = std::min<int64_t>(f + q.spanLen[k], window);
        return *a0 < *a1;
    };

    MRC_TRY(ensure_decode_consts(h));
    StoreBufs& b = h->store;
    MRC_HIP(h, b.ev.create());
    hipStream_t st = pick_stream(h, q.stream);
    DrainGuard drain{{st, nullptr, nullptr}};
    const size_t elem = format == MRC_WINDOW_PCM16 ? 2 : format == MRC_WINDOW_F32 ? 4 : 8;
    const ResampleTable* table = nullptr;
    if (rs) MRC_TRY(get_resample_table(h, *rs, &table));
    const int64_t up = rs ? rs->up : 1, down = rs ? rs->down : 1, W = rs ? rs->W : 0;
    int64_t span = rs ? ((window - 1) * down + up - 1) / up + 2 * W : window;           // plane samples a unit takes at most
    const ResampleTable* tables[MRC_MAX_STORE_RATIOS] = {};
    SpeedRatio ratios[MRC_MAX_STORE_RATIOS] = {};
    if (speeds) {                                            // every filter first, then the largest span among the ratios named
        MRC_TRY(get_resample_tables(h, speeds->nRatios, speeds->r, tables));
        for (int i = 0; i < speeds->nRatios; ++i) {
            const ResampleSpec& r = speeds->r[i];
            ratios[i] = SpeedRatio{r.up, r.down, r.W, r.W ? tables[i]->skewNatural : 0, r.W ? (const double*)tables[i]->taps.p : nullptr};
        }
        span = 0;
        for (int64_t k = unitsBefore(run.first); k < unitsBefore(run.last); ++k) {
            const ResampleSpec& r = speeds->r[q.ratioOf[k]];
            span = std::max<int64_t>(span, r.W ? ((window - 1) * r.down + r.up - 1) / r.up + 2 * r.W : window);
        }
    }
    if (spans) {                                             // planes as long as the range's longest span asks, not as the window
        span = 0;
        for (int64_t k = unitsBefore(run.first), a0, a1; k < unitsBefore(run.last); ++k) {
            if (!audible(k, &a0, &a1)) continue;
            const ResampleSpec* r = rs ? rs : speeds && speeds->r[q.ratioOf[k]].W ? &speeds->r[q.ratioOf[k]] : nullptr;
            span = std::max<int64_t>(span, r ? ((a1 - a0 - 1) * r->down + r->up - 1) / r->up + 2 * r->W : a1 - a0);
        }
    }
    const int64_t far = (int64_t)1 << 52;                    // an output start beyond it is beyond every file: (start + window) * down fits
    const int64_t planeLen = span + 4 * L, tiles = (window + 255) / 256;
    const int64_t slab = run.slab, itemCap = std::max<int64_t>(1, 0x7fffffffLL / (tiles * n_channels_out));

    std::vector<Need>& needs = b.needs;                      // (the planner's scratch: StoreBufs)
    std::vector<WindowItem>& items = b.items;
    PacPlan pl;                                              // (its group fields: the slab's slots)
    for (int64_t first = run.first, last; first < run.last; first = last) {  // rows [first, last), their units [u0, u0 + nSlab)
        last = first + 1;
        while (last < run.last && last - first < itemCap && (slab == 0 || (unitsBefore(last + 1) - unitsBefore(first)) * span <= slab)) ++last;
        const int64_t nSlabRows = last - first, u0 = unitsBefore(first), nSlab = unitsBefore(last) - u0;
        unsigned char* outSlab = (unsigned char*)run.out + (size_t)(first - run.first) * n_channels_out * window * elem;
        s->stats[2] += 1;

        // ---- the slab's needed blocks, its items and planes
        needs.clear();
        items.assign((size_t)nSlab, WindowItem{0, 0, 0, 1, 0});
        int64_t planeDoubles = 0;
        for (int64_t k = 0; k < nSlab; ++k) {
            const int64_t f = file[u0 + k];
            const size_t before = needs.size();
            const int64_t outStart = startOf(u0 + k);
            int64_t a0, a1;                                  // the row samples the term gives: all of them without spans
            if (!audible(u0 + k, &a0, &a1)) continue;        // silent in this row: no block, no plane, nothing parsed
            if (spans && (outStart > far || outStart < -far)) continue;      // (beyond every file; outStart + a0 is then safe to form)
            int64_t at = outStart + a0, len = a1 - a0;       // the samples the planes must hold: [at, at + len)
            if (rs) {
                if (at > far || at < -far) continue;
                at = floor_div(at * down, up) - W + 1;
                len = floor_div((outStart + a1 - 1) * down, up) + W - at + 1;
            } else if (speeds && speeds->r[q.ratioOf[u0 + k]].W) {
                const ResampleSpec& r = speeds->r[q.ratioOf[u0 + k]];
                if (at > far || at < -far) continue;
                at = floor_div(at * r.down, r.up) - r.W + 1;
                len = floor_div((outStart + a1 - 1) * r.down, r.up) + r.W - at + 1;
            }
            needed_blocks(*s, cfg, D, k, f, at, len, &needs);
            if (needs.size() == before) continue;            // all zeros: its plane does not exist
            const PacFilePlan& fi = s->index.files[(size_t)f];
            const int nPlanes = mix == kNoMix ? fi.nch : 1;
            items[(size_t)k] = WindowItem{planeDoubles, at, std::max<int64_t>(0, fi.total - cfg.n_mdct_lines) / D, nPlanes, 0};
            planeDoubles += nPlanes * planeLen;
        }
        if (needs.empty()) {                                 // nothing to decode: zeros, no launch
            MRC_HIP(h, hipMemsetAsync(outSlab, 0, (size_t)nSlabRows * n_channels_out * window * elem, st));
            continue;
        }
        // ---- staging (one H2D copy): plan | groups | block offsets | items (a sum: term records | the rows' term offsets);
        // a slot's offset is its block's place in the item's plane: the block's position in the file's padded plane, the
        // window's start at 2 L
        size_t oOffs = 0, oItems = 0, oOutStart = 0, oLineBand = 0, oBandGain = 0, oUnit = 0, oRatioOf = 0, oRatios = 0, oSpans = 0;
        SlabStage S;
        MRC_TRY(stage_slab(
            s, fn, mix, needs, &pl, &S,
            [&](StageLayout* lay) {
                oOffs = lay->add<long long>(pl.totalSlots);
                if (sum) {
                    oItems = lay->add<SumTerm>(nSlab);
                    oOutStart = lay->add<long long>(nSlabRows + 1);      // (the rows' term offsets, from the slab's first term)
                } else {
                    oItems = lay->add<WindowItem>(nSlab);
                    if (rs) oOutStart = lay->add<long long>(nSlab);
                }
                if (shape) {
                    oLineBand = lay->add<uint16_t>((int64_t)shape->lineBand.size());
                    oBandGain = lay->add<double>(nSlab * q.nBands);
                    oUnit = lay->add<int>(pl.totalSlots);    // (indexed as the offsets are: a pair's workgroup, a single slot)
                }
                if (speeds) {
                    oRatioOf = lay->add<int>(nSlab);
                    oRatios = lay->add<SpeedRatio>(speeds->nRatios);
                }
                if (spans) oSpans = lay->add<TermSpan>(nSlab);
            },
            [&](const Need& n, int g, int slot, int ch, bool pair) {
                const WindowItem& it = items[(size_t)n.item];
                long long* offs = (long long*)(S.pin + oOffs) + pl.slotBase[g];
                const int64_t at = it.plane + 2 * L + s->blockStart[(size_t)(s->firstBlock[(size_t)n.file] + n.block)] / D - (it.start + L);
                // a pair's workgroup is its index among the pairs; a single slot's comes after the group's pairs; without a
                // mix a channel has a plane of its own
                const int64_t wg = pair ? slot / 2 : slot - S.nPairs[g];
                offs[wg] = pair ? at : at + (mix == kNoMix ? ch * planeLen : 0);
                if (shape) ((int*)(S.pin + oUnit))[pl.slotBase[g] + wg] = (int)n.item;
            }));
        const int64_t* nPairs = S.nPairs;
        const UnpackGroupDev* gd = S.gd;
        if (sum) {
            SumTerm* terms = (SumTerm*)(S.pin + oItems);
            const auto resampled = [&](int64_t k) { return rs || (speeds && speeds->r[q.ratioOf[u0 + k]].W); };
            for (int64_t k = 0; k < nSlab; ++k)
                terms[k] = SumTerm{items[(size_t)k], run.termRows ? 1.0 : q.gain[u0 + k], resampled(k) ? startOf(u0 + k) : 0};
            long long* slabTerms = (long long*)(S.pin + oOutStart);
            for (int64_t r = 0; r <= nSlabRows; ++r) slabTerms[r] = unitsBefore(first + r) - u0;
        } else {
            std::memcpy(S.pin + oItems, items.data(), sizeof(WindowItem) * nSlab);
            if (rs) std::memcpy(S.pin + oOutStart, q.start + first, sizeof(long long) * nSlab);
        }
        if (spans) {                                         // (spans come with rows: the records lie beside the SumTerms)
            TermSpan* sp = (TermSpan*)(S.pin + oSpans);
            for (int64_t k = 0, a0, a1; k < nSlab; ++k) {
                audible(u0 + k, &a0, &a1);
                sp[k] = TermSpan{q.spanFirst[u0 + k] + run.preRoll, q.spanLen[u0 + k], q.fadeIn ? q.fadeIn[u0 + k] : 0,
                                 q.fadeOut ? q.fadeOut[u0 + k] : 0, a0};
            }
        }
        if (speeds) {
            int* ratioOf = (int*)(S.pin + oRatioOf);
            for (int64_t k = 0; k < nSlab; ++k) ratioOf[k] = q.ratioOf[u0 + k];
            std::memcpy(S.pin + oRatios, ratios, sizeof(SpeedRatio) * (size_t)speeds->nRatios);
        }
        if (shape) {
            std::memcpy(S.pin + oLineBand, shape->lineBand.data(), sizeof(uint16_t) * shape->lineBand.size());
            std::memcpy(S.pin + oBandGain, q.bandGain + u0 * q.nBands, sizeof(double) * (size_t)(nSlab * q.nBands));
        }
        const HostShape* reduced[4] = {};
        for (int sh = 0; D > 1 && sh < 4; ++sh)
            if (pl.hs[sh]) MRC_TRY(get_synth_shape(h, pl.hs[sh]->dev.a, pl.hs[sh]->dev.b, D, &reduced[sh]));
        MRC_HIP(h, b.planes.reserve(sizeof(double) * (size_t)planeDoubles));

        // ---- device: the parse step (the plan entries point into the resident bytes), then one launch per group with slots
        unsigned char* din = b.in.as<unsigned char>();
        MRC_TRY(parse_slab(s, fn, S, st));
        double* x = b.planes.as<double>();
        MRC_HIP(h, hipEventRecord(b.ev[3], st));
        MRC_HIP(h, hipMemsetAsync(x, 0, sizeof(double) * (size_t)planeDoubles, st));
        const int64_t* offsDev = (const int64_t*)(din + oOffs);
        if (shape)
            MRC_TRY(pac_for_groups(h, pl, gd, offsDev, [&](int g, const UnpackGroupDev& G, const int64_t* o) {
                const DevShape& F = pl.hs[g / 2]->dev;
                const DevShape* R = D == 1 ? nullptr : &reduced[g / 2]->dev;
                const uint16_t* lineBand = (const uint16_t*)(din + oLineBand) + shape->lineOff[g / 2];
                const double* bandGain = (const double*)(din + oBandGain);
                const int* unit = (const int*)(din + oUnit) + (o - offsDev);
                if (mix != kNoMix)
                    return launch_decode_shaped_mix(F, R, lineBand, bandGain, unit, q.nBands, pl.nSlots[g] - nPairs[g], G.joint,
                                                    mix == MRC_MIX_MID ? 2 : mix == MRC_MIX_LEFT ? 0 : 1, nPairs[g], G.oscale,
                                                    G.joint ? G.ms : nullptr, G.sf, G.ba, G.mant, o, x, st);
                return launch_decode_shaped(F, R, lineBand, bandGain, unit, q.nBands, pl.nSlots[g], G.joint ? 2 : 1, G.oscale,
                                            G.joint ? G.ms : nullptr, G.sf, G.ba, G.mant, o, x, G.joint ? x + planeLen : nullptr, st);
            }));
        else if (mix == kNoMix && D == 1) MRC_TRY(decode_groups(h, pl, gd, offsDev, x, planeLen, st));
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
        // spans come with a list of ratios (the reverb and STFT entries' arguments).  A list of ONE ratio goes to the single-ratio
        // kernels -- the bits are the same, a fold's order being per output, and a ratio like 3 / 2 keeps its evenOdd LDS layout
        const TermSpan* spansDev = (const TermSpan*)(din + oSpans);
        const ResampleSpec* one = spans && speeds && speeds->nRatios == 1 ? &speeds->r[0] : nullptr;
        if (one && one->W == 0)
            MRC_HIP(h, launch_span_sum_out(nSlabRows, (const SumTerm*)(din + oItems), spansDev, (const long long*)(din + oOutStart), window,
                                           n_channels_out, format, (int)L, planeLen, x, outSlab, st));
        else if (one)
            MRC_HIP(h, launch_span_resample_sum_out(nSlabRows, (const SumTerm*)(din + oItems), spansDev, (const long long*)(din + oOutStart),
                                                    window, n_channels_out, format, (int)L, planeLen, one->up, one->down, one->W,
                                                    tables[0]->evenOdd, tables[0]->skew, (const double*)tables[0]->taps.p, x, outSlab, st));
        else if (spans)
            MRC_HIP(h, launch_span_resample_multi_sum_out(nSlabRows, (const SumTerm*)(din + oItems), spansDev, (const int*)(din + oRatioOf),
                                                          (const SpeedRatio*)(din + oRatios), ratios, speeds->nRatios,
                                                          (const long long*)(din + oOutStart), window, n_channels_out, format, (int)L,
                                                          planeLen, x, outSlab, st));
        else if (speeds)
            MRC_HIP(h, launch_resample_multi_sum_out(nSlabRows, (const SumTerm*)(din + oItems), (const int*)(din + oRatioOf),
                                                     (const SpeedRatio*)(din + oRatios), ratios, speeds->nRatios,
                                                     (const long long*)(din + oOutStart), window, n_channels_out, format, (int)L,
                                                     planeLen, x, outSlab, st));
        else if (sum && rs)
            MRC_HIP(h, launch_resample_sum_out(nSlabRows, (const SumTerm*)(din + oItems), (const long long*)(din + oOutStart), window,
                                               n_channels_out, format, (int)L, planeLen, rs->up, rs->down, rs->W, table->evenOdd,
                                               table->skew, (const double*)table->taps.p, x, outSlab, st));
        else if (sum)
            MRC_HIP(h, launch_sum_out(nSlabRows, (const SumTerm*)(din + oItems), (const long long*)(din + oOutStart), window,
                                      n_channels_out, format, (int)L, x, outSlab, st));
        else if (rs)
            MRC_HIP(h, launch_resample_out(nSlab, (const WindowItem*)(din + oItems), (const long long*)(din + oOutStart), window,
                                           n_channels_out, format, (int)L, planeLen, rs->up, rs->down, rs->W, table->evenOdd,
                                           table->skew, (const double*)table->taps.p, x, outSlab, st));
        else
            MRC_HIP(h, launch_window_out(nSlab, (const WindowItem*)(din + oItems), window, n_channels_out, format, (int)L, x,
                                         outSlab, st));
        MRC_HIP(h, hipEventRecord(b.ev[5], st));
        MRC_HIP(h, hipStreamSynchronize(st));                // (the staging is written again by the next slab)
        MRC_TRY(add_elapsed(h, b.ev, kSlabSpans, 4, s->ms));
    }
    MRC_HIP(h, hipStreamSynchronize(st));
    return MRC_OK;
}

// the per-group entries of a slab into its staging at dst, group after group; entryBase[g]: where group g's start -> their number
int64_t copy_entries(const std::vector<EnergyEntry>* entries, unsigned char* dst, int64_t* entryBase) {
    int64_t q = 0;
    for (int g = 0; g < kUnpackGroups; ++g) {
        entryBase[g] = q;
        if (!entries[g].empty())
            std::memcpy(dst + sizeof(EnergyEntry) * (size_t)q, entries[g].data(), sizeof(EnergyEntry) * entries[g].size());
        q += (int64_t)entries[g].size();
    }
    return q;
}

// mrc_pac_store_block_energy: every block of the selected files through the slab's parse (stage_slab, parse_slab: the
// planner of units_loop) and block_energy_kernel, one launch per group with slots; no plane, no inverse transform.
// A slab is a run of whole blocks, in the order of the entries, whose b / D sum to at most MRC_OPT_STORE_SLAB_SAMPLES (one
// block at least): its entries are consecutive, so its energies come back in one copy.
struct BlockEnergyRequest {                                  // the entry's arguments, as the header names them
    int rate_divisor, mix;
    int64_t n_sel;
    const int64_t* file;
    int64_t* entry_offset;
    int64_t entry_cap;
    int64_t* entry_block;
    double* energy;
    void* stream;
};
int block_energy(mrc_pac_store* s, const BlockEnergyRequest& r) {
    const char* const fn = "mrc_pac_store_block_energy";
    const int D = r.rate_divisor, mixArg = r.mix;
    const int64_t n_sel = r.n_sel, entry_cap = r.entry_cap, *const file = r.file;
    int64_t *const entry_offset = r.entry_offset, *const entry_block = r.entry_block;
    double* const energy = r.energy;
    MRC_TRY(store_alive(s, fn));
    mrc_handle* h = s->h;
    const mrc_config& cfg = h->cfg;
    const std::string w = fn;
    reset_stats(s);
    MRC_TRY(check_mix(h, w, mixArg, kMixEachOrMid));
    const int mix = mixArg == MRC_MIX_MID ? MRC_MIX_MID : kNoMix;
    MRC_TRY(check_divisor(h, w, D));
    const int64_t nFiles = (int64_t)s->index.files.size();
    if (n_sel < 0) return fail(h, MRC_ERR_INVALID, w + ": n_sel < 0");
    if (!file && n_sel != nFiles)
        return fail(h, MRC_ERR_INVALID, w + ": file is NULL (every file in order) but n_sel = " + std::to_string(n_sel) + " is not the store's " +
                                            std::to_string(nFiles) + " files");
    if (!entry_offset) return fail(h, MRC_ERR_INVALID, w + ": entry_offset is NULL");
    if (entry_cap < 0) return fail(h, MRC_ERR_INVALID, w + ": entry_cap < 0");
    const auto fileOf = [file](int64_t k) { return file ? file[k] : k; };
    MRC_TRY(check_files(s, w, n_sel, file, 0, "item"));
    const auto columns = [&](int64_t f) { return mix == kNoMix ? s->index.files[(size_t)f].nch : 1; };
    entry_offset[0] = 0;
    for (int64_t k = 0; k < n_sel; ++k) entry_offset[k + 1] = entry_offset[k] + s->index.nBlocks(fileOf(k)) * columns(fileOf(k));
    const int64_t nEntries = entry_offset[n_sel];
    if (nEntries > entry_cap)
        return fail(h, MRC_ERR_NOMEM, w + ": entry_cap = " + std::to_string(entry_cap) + " is too small for " + std::to_string(nEntries) + " entries");
    if (nEntries == 0) return MRC_OK;
    if (!energy) return fail(h, MRC_ERR_INVALID, w + ": energy is NULL");

    MRC_TRY(ensure_decode_consts(h));
    StoreBufs& b = h->store;
    MRC_HIP(h, b.ev.create());
    hipStream_t st = pick_stream(h, r.stream);
    DrainGuard drain{{st, nullptr, nullptr}};
    const int64_t slab = h->storeSlabSamples, blockCap = (int64_t)1 << 28;      // (entries and slots of a launch stay below 2^31)

    std::vector<Need>& needs = b.needs;                      // (the planner's scratch: StoreBufs)
    std::vector<EnergyEntry>(&entries)[kUnpackGroups] = b.entries;
    PacPlan pl;                                              // (its group fields: the slab's slots)
    int64_t k = 0, blk = 0;                                  // the next block: block blk of selection k
    while (k < n_sel && s->index.nBlocks(fileOf(k)) == 0) ++k;
    while (k < n_sel) {
        // ---- the slab's blocks, from (k, blk) on
        needs.clear();
        const int64_t firstEntry = entry_offset[k] + blk * columns(fileOf(k));
        int64_t nSlabEntries = 0;
        for (int64_t samples = 0; k < n_sel;) {
            const int64_t f = fileOf(k);
            int a, bb;
            shape_ab(cfg, s->index.shape(f, blk), &a, &bb);
            if (!needs.empty() && ((slab != 0 && samples + bb / D > slab) || (int64_t)needs.size() >= blockCap)) break;
            samples += bb / D;
            needs.push_back(Need{k, f, blk});
            nSlabEntries += columns(f);
            if (entry_block) {
                const int64_t p = s->blockStart[(size_t)(s->firstBlock[(size_t)f] + blk)];
                for (int64_t e = entry_offset[k] + blk * columns(f), c = 0; c < columns(f); ++c, ++e) {
                    entry_block[3 * e] = p;
                    entry_block[3 * e + 1] = a;
                    entry_block[3 * e + 2] = bb;
                }
            }
            if (++blk == s->index.nBlocks(f)) {
                blk = 0;
                do ++k; while (k < n_sel && s->index.nBlocks(fileOf(k)) == 0);
            }
        }
        s->stats[2] += 1;

        // ---- staging (one H2D copy): plan | groups | entries, group after group
        for (auto& v : entries) v.clear();
        size_t oEntries = 0;
        SlabStage S;
        MRC_TRY(stage_slab(
            s, fn, mix, needs, &pl, &S, [&](StageLayout* lay) { oEntries = lay->add<EnergyEntry>(nSlabEntries); },
            [&](const Need& n, int g, int slot, int ch, bool pair) {
                const long long out = entry_offset[n.item] + n.block * columns(n.file) - firstEntry;
                const bool joint = !(g & 1);
                if (mix == MRC_MIX_MID) {                    // one entry per block: a joint slot, a pair (at its first slot) or a mono slot
                    if (!pair || ch == 0) entries[g].push_back(EnergyEntry{out, slot, joint || pair ? kEnergyMid : 0});
                } else if (joint) {
                    for (int c = 0; c < 2; ++c) entries[g].push_back(EnergyEntry{out + c, slot, c});
                } else {
                    entries[g].push_back(EnergyEntry{out + ch, slot, 0});
                }
            }));
        int64_t entryBase[kUnpackGroups];
        if (copy_entries(entries, S.pin + oEntries, entryBase) != nSlabEntries)
            return fail(h, MRC_ERR_INVALID, w + ": internal error: a slab's entries do not add up");
        MRC_HIP(h, b.planes.reserve(sizeof(double) * (size_t)nSlabEntries));

        // ---- device: the parse step, one block_energy_kernel launch per group with slots, the energies back
        MRC_TRY(parse_slab(s, fn, S, st));
        double* e = b.planes.as<double>();
        const EnergyEntry* entDev = (const EnergyEntry*)(b.in.as<unsigned char>() + oEntries);
        MRC_HIP(h, hipEventRecord(b.ev[3], st));
        for (int g = 0; g < kUnpackGroups; ++g) {
            if (entries[g].empty()) continue;
            const UnpackGroupDev& G = S.gd[g];
            MRC_HIP(h, launch_block_energy(pl.hs[g / 2]->dev, D, G.joint, (int64_t)entries[g].size(), entDev + entryBase[g], G.oscale,
                                           G.joint ? G.ms : nullptr, G.sf, G.ba, G.mant, e, st));
            s->stats[1] += 1;
        }
        MRC_HIP(h, hipEventRecord(b.ev[4], st));
        MRC_HIP(h, hipMemcpyAsync(energy + firstEntry, e, sizeof(double) * (size_t)nSlabEntries, hipMemcpyDeviceToHost, st));
        MRC_HIP(h, hipStreamSynchronize(st));                // (the staging is written again by the next slab)
        MRC_TRY(add_elapsed(h, b.ev, kSlabSpans, 3, s->ms));
    }
    return MRC_OK;
}

// mrc_band_line_ranges' rule; the refusal's words (the caller puts its own name in front), empty if there is none
std::string band_line_ranges(double sampleRate, int a, int b, int nBands, const double* edge, int32_t* lineLo) {
    if (nBands < 1 || nBands > MRC_MAX_STORE_BANDS)
        return "n_bands " + std::to_string(nBands) + " is outside 1.." + std::to_string(MRC_MAX_STORE_BANDS);
    if (!edge || !lineLo) return "edge_hz or line_lo is NULL";
    for (int q = 0; q <= nBands; ++q)
        if (!std::isfinite(edge[q])) return "edge_hz[" + std::to_string(q) + "] is not finite";
    if (edge[0] < 0) return "edge_hz[0] < 0";
    for (int q = 0; q < nBands; ++q)
        if (!(edge[q] < edge[q + 1])) return "edge_hz is not strictly increasing at [" + std::to_string(q + 1) + "]";
    if (!(sampleRate > 0) || !std::isfinite(sampleRate)) return "sample_rate is not a positive number";
    const std::string refusal = synth_shape_refusal(a, b, 1);
    if (!refusal.empty()) return refusal;
    const int halfN = (a + b) / 2;
    int k = 0;                                               // f_k does not decrease with k: one pass over lines and edges
    for (int q = 0; q <= nBands; ++q) {
        while (k < halfN && (k + 0.5) * ((sampleRate / halfN) / 2.) < edge[q]) ++k;      // psychoac.py:94, 99
        lineLo[q] = k;
    }
    return std::string();
}

// mrc_filterbank_line_weights' rule; rows (may be null: sizes only) receives the weights, filter after filter.  The
// refusal's words as band_line_ranges gives them.  Host float64 in the header's order of operations (-ffp-contract=off).
struct FilterPoints { double sampleRate; int nFilters; const double* p; int norm; };
std::string filterbank_line_weights(const FilterPoints& bank, int a, int b, int32_t* lineLo, int32_t* lineHi, std::vector<double>* rows,
                                    int64_t* nWeights) {
    const double sampleRate = bank.sampleRate, *p = bank.p;
    const int nFilters = bank.nFilters, norm = bank.norm;
    if (nFilters < 1 || nFilters > MRC_MAX_STORE_BANDS)
        return "n_filters " + std::to_string(nFilters) + " is outside 1.." + std::to_string(MRC_MAX_STORE_BANDS);
    if (!p || !lineLo || !lineHi || !nWeights) return "point_hz, line_lo, line_hi or n_weights is NULL";
    for (int q = 0; q < nFilters + 2; ++q)
        if (!std::isfinite(p[q])) return "point_hz[" + std::to_string(q) + "] is not finite";
    if (p[0] < 0) return "point_hz[0] < 0";
    for (int q = 0; q < nFilters + 1; ++q)
        if (!(p[q] < p[q + 1])) return "point_hz is not strictly increasing at [" + std::to_string(q + 1) + "]";
    if (norm != MRC_FILTER_NORM_NONE && norm != MRC_FILTER_NORM_SLANEY)
        return "norm " + std::to_string(norm) + " is not MRC_FILTER_NORM_NONE (0) or MRC_FILTER_NORM_SLANEY (1)";
    if (!(sampleRate > 0) || !std::isfinite(sampleRate)) return "sample_rate is not a positive number";
    const std::string refusal = synth_shape_refusal(a, b, 1);
    if (!refusal.empty()) return refusal;
    const int halfN = (a + b) / 2;
    const double d = (sampleRate / halfN) / 2.;
    int kl = 0, kh = 0;                                      // e_k does not decrease with k, nor the points with q: one pass
    int64_t total = 0;
    for (int q = 0; q < nFilters; ++q) {
        const double p0 = p[q], p1 = p[q + 1], p2 = p[q + 2];
        while (kl < halfN && (double)(kl + 1) * d <= p0) ++kl;
        while (kh < halfN && (double)kh * d < p2) ++kh;
        lineLo[q] = kl;
        lineHi[q] = std::max(kl, kh);                        // (kl <= kh: line kl starts at or below p0 < p2, or kl is halfN)
        total += lineHi[q] - lineLo[q];
        if (!rows) continue;
        for (int k = lineLo[q]; k < lineHi[q]; ++k) {
            const double f0 = (double)k * d, f1 = (double)(k + 1) * d;
            const double u0 = std::max(f0, p0), u1 = std::min(f1, p1);
            const double rise = u1 > u0 ? ((0.5 * (u0 + u1) - p0) / (p1 - p0)) * (u1 - u0) : 0.0;
            const double v0 = std::max(f0, p1), v1 = std::min(f1, p2);
            const double fall = v1 > v0 ? ((p2 - 0.5 * (v0 + v1)) / (p2 - p1)) * (v1 - v0) : 0.0;
            double w = (rise + fall) / d;
            if (norm == MRC_FILTER_NORM_SLANEY) w = w * (2.0 / (p2 - p0));
            rows->push_back(w);
        }
    }
    *nWeights = total;
    return std::string();
}

// What differs between mrc_pac_store_band_energy_window and mrc_pac_store_filterbank_window: the per-shape table, which
// rides in every slab's staging copy as 8-byte words, and the launcher called per (shape, kind) group.
struct EnergyTable {
    const char* fn;                                          // the entry point's name, in front of every refusal
    int nOut;                                                // bands or filters: the rows of an output channel
    // fills words for the handle's four shapes, once per call; the refusal's words, empty if there is none
    std::function<std::string(const mrc_config&)> build;
    std::vector<int64_t> words;
    // sums[entry.out][nOut] of one group's entries; table: words on the device
    std::function<hipError_t(int shape, const DevShape& F, const UnpackGroupDev& G, const int64_t* table, int64_t nEntries,
                             const EnergyEntry* entries, double* sums, hipStream_t st)> launch;
};

// mrc_pac_store_band_energy_window and mrc_pac_store_filterbank_window: the slab's parse (stage_slab, parse_slab) over the
// blocks whose TILES the items' frames overlap, the table's kernel per group with slots into B [rows][nOut] in the store
// workspace, band_frames_kernel over the slab's output.  An item's rows are its needed blocks in file order, a row per
// decoded channel.
struct FramesRequest {                                       // the arguments the two entries share, as the header names them
    int mix;
    int64_t n_items;
    const int64_t *file, *start;
    int64_t n_frames, hop;
    int n_channels_out, format;
    void *out, *stream;
};
int energy_frames_window(mrc_pac_store* s, EnergyTable& T, const FramesRequest& r) {
    const char* const fn = T.fn;
    const int n_bands = T.nOut, mixArg = r.mix, n_channels_out = r.n_channels_out, format = r.format;
    const int64_t n_items = r.n_items, n_frames = r.n_frames, hop = r.hop, *file = r.file, *start = r.start;
    void *const out = r.out, *const stream = r.stream;
    MRC_TRY(store_alive(s, fn));
    mrc_handle* h = s->h;
    const mrc_config& cfg = h->cfg;
    const std::string w = fn;
    reset_stats(s);
    MRC_TRY(check_mix(h, w, mixArg, kMixAny));
    const int mix = mixArg == MRC_MIX_EACH ? kNoMix : mixArg;
    if (mix == kNoMix ? n_channels_out != 1 && n_channels_out != 2 : n_channels_out != 1)
        return fail(h, MRC_ERR_INVALID, w + (mix == kNoMix ? ": n_channels_out must be 1 or 2" : ": n_channels_out must be 1 under a mix of one channel"));
    if (format != MRC_WINDOW_F32 && format != MRC_WINDOW_F64)
        return fail(h, MRC_ERR_INVALID, w + ": format " + std::to_string(format) + " is not MRC_WINDOW_F32 (1) or MRC_WINDOW_F64 (2)");
    if (n_items < 0) return fail(h, MRC_ERR_INVALID, w + ": n_items < 0");
    if (n_frames < 0) return fail(h, MRC_ERR_INVALID, w + ": n_frames < 0");
    if (hop < 1) return fail(h, MRC_ERR_INVALID, w + ": hop < 1");
    if (n_frames > ((int64_t)1 << 62) / hop) return fail(h, MRC_ERR_INVALID, w + ": n_frames * hop is above 2^62");
    {
        const std::string refusal = T.build(cfg);
        if (!refusal.empty()) return fail(h, MRC_ERR_INVALID, w + ": " + refusal);
    }
    const int64_t span = n_frames * hop;
    if (n_items > 0 && (!file || !start)) return fail(h, MRC_ERR_INVALID, w + ": file or start is NULL");
    if (n_items > 0 && n_frames > 0 && !out) return fail(h, MRC_ERR_INVALID, w + ": out is NULL");
    MRC_TRY(check_files(s, w, n_items, file, mix == kNoMix ? n_channels_out : 0, "item"));
    if (n_items == 0 || n_frames == 0) return MRC_OK;

    MRC_TRY(ensure_decode_consts(h));
    StoreBufs& b = h->store;
    MRC_HIP(h, b.ev.create());
    hipStream_t st = pick_stream(h, stream);
    DrainGuard drain{{st, nullptr, nullptr}};
    const size_t elem = format == MRC_WINDOW_F32 ? 4 : 8;
    const int64_t rowLen = (int64_t)n_channels_out * n_bands * n_frames;     // one item's output values
    const int64_t slab = h->storeSlabSamples, itemCap = std::max<int64_t>(1, ((int64_t)1 << 38) / rowLen);   // (a launch's grid below 2^31)
    const auto floorHalf = [](int64_t v) { return v >= 0 ? v / 2 : -((-v + 1) / 2); };

    std::vector<Need>& needs = b.needs;                      // (the planner's scratch: StoreBufs)
    std::vector<BandItem>& items = b.bandItems;
    std::vector<int64_t>& firstTile = b.firstTile;           // per item: its first needed block
    std::vector<EnergyEntry>(&entries)[kUnpackGroups] = b.entries;
    PacPlan pl;                                              // (its group fields: the slab's slots)
    for (int64_t first = 0, last; first < n_items; first = last) {
        last = first + 1;
        while (last < n_items && last - first < itemCap && (slab == 0 || span <= slab / (last - first + 1))) ++last;
        const int64_t nSlab = last - first;
        unsigned char* outSlab = (unsigned char*)out + (size_t)first * (size_t)rowLen * elem;
        s->stats[2] += 1;

        // ---- the slab's items: the run of blocks whose tile overlaps [start, start + span), in doubled samples
        // [2 start, 2 (start + span)) against the file's ascending edges; compared without doubling an extreme start
        needs.clear();
        items.assign((size_t)nSlab, BandItem{0, 0, 0, 0, 0, 0, 1});
        firstTile.assign((size_t)nSlab, 0);
        int64_t nRows = 0, nEdges = 0;
        for (int64_t k = 0; k < nSlab; ++k) {
            const int64_t f = file[first + k], nb = s->index.nBlocks(f), at = start[first + k];
            if (nb == 0) continue;
            const int64_t* E = s->tileEdge.data() + s->firstBlock[(size_t)f] + f;
            const int64_t lo = floorHalf(E[0]), hi = floorHalf(E[nb]) + 1;       // lo <= E / 2 <= hi for every edge
            if (at >= hi || (at < lo && lo - at >= span)) continue;              // behind the last tile, or ends before the first
            const int64_t s2 = 2 * std::max(at, lo), e2 = 2 * std::min(at + span, hi);      // (at < hi: at + span fits)
            const int64_t b0 = std::upper_bound(E + 1, E + nb + 1, s2) - (E + 1);           // first tile that ends behind s2
            const int64_t b1 = std::lower_bound(E, E + nb, e2) - E;                         // first tile that starts at or behind e2
            if (b0 >= b1) continue;
            const int cols = mix == kNoMix ? s->index.files[(size_t)f].nch : 1;
            items[(size_t)k] = BandItem{nEdges, nRows, at, lo, hi, (int)(b1 - b0), cols};
            firstTile[(size_t)k] = b0;
            for (int64_t i = b0; i < b1; ++i) needs.push_back(Need{k, f, i});
            nRows += (b1 - b0) * cols;
            nEdges += b1 - b0 + 1;
        }
        if (needs.empty()) {                                 // no tile under any frame: zeros, no launch
            MRC_HIP(h, hipMemsetAsync(outSlab, 0, (size_t)nSlab * (size_t)rowLen * elem, st));
            continue;
        }
        // ---- staging (one H2D copy): plan | groups | entries, group after group | line tables | tile edges | items
        for (auto& v : entries) v.clear();
        size_t oEntries = 0, oLines = 0, oEdges = 0, oItems = 0;
        int64_t nSlabEntries = 0;
        SlabStage S;
        MRC_TRY(stage_slab(
            s, fn, mix, needs, &pl, &S,
            [&](StageLayout* lay) {
                for (const Need& n : needs) nSlabEntries += mix == kNoMix ? s->index.files[(size_t)n.file].nch : 1;
                oEntries = lay->add<EnergyEntry>(nSlabEntries);
                oLines = lay->add<int64_t>(T.words.size());
                oEdges = lay->add<long long>(nEdges);
                oItems = lay->add<BandItem>(nSlab);
            },
            [&](const Need& n, int g, int slot, int ch, bool pair) {
                const BandItem& it = items[(size_t)n.item];
                const long long row = it.row0 + (n.block - firstTile[(size_t)n.item]) * it.nch;
                const bool joint = !(g & 1);
                if (mix == MRC_MIX_MID) {                    // one entry per block: a joint slot, a pair (at its first slot) or a mono slot
                    if (!pair || ch == 0) entries[g].push_back(EnergyEntry{row, slot, joint || pair ? kEnergyMid : 0});
                } else if (joint) {
                    if (mix == kNoMix) for (int c = 0; c < 2; ++c) entries[g].push_back(EnergyEntry{row + c, slot, c});
                    else entries[g].push_back(EnergyEntry{row, slot, mix == MRC_MIX_LEFT ? 0 : 1});
                } else {
                    entries[g].push_back(EnergyEntry{row + (mix == kNoMix ? ch : 0), slot, 0});
                }
            }));
        int64_t entryBase[kUnpackGroups];
        const int64_t q = copy_entries(entries, S.pin + oEntries, entryBase);
        if (q != nSlabEntries || q != nRows) return fail(h, MRC_ERR_INVALID, w + ": internal error: a slab's entries do not add up");
        std::memcpy(S.pin + oLines, T.words.data(), sizeof(int64_t) * T.words.size());
        long long* edges = (long long*)(S.pin + oEdges);
        for (int64_t k = 0; k < nSlab; ++k) {
            const BandItem& it = items[(size_t)k];
            if (it.nTiles == 0) continue;
            const int64_t f = file[first + k];
            const int64_t* E = s->tileEdge.data() + s->firstBlock[(size_t)f] + f + firstTile[(size_t)k];
            for (int64_t i = 0; i <= it.nTiles; ++i) edges[it.edge0 + i] = E[i];
        }
        std::memcpy(S.pin + oItems, items.data(), sizeof(BandItem) * (size_t)nSlab);
        MRC_HIP(h, b.planes.reserve(sizeof(double) * (size_t)nRows * (size_t)n_bands));

        // ---- device: the parse step, one launch of the table's kernel per group with slots, the frames
        MRC_TRY(parse_slab(s, fn, S, st));
        unsigned char* din = b.in.as<unsigned char>();
        double* B = b.planes.as<double>();
        const EnergyEntry* entDev = (const EnergyEntry*)(din + oEntries);
        MRC_HIP(h, hipEventRecord(b.ev[3], st));
        for (int g = 0; g < kUnpackGroups; ++g) {
            if (entries[g].empty()) continue;
            const UnpackGroupDev& G = S.gd[g];
            MRC_HIP(h, T.launch(g / 2, pl.hs[g / 2]->dev, G, (const int64_t*)(din + oLines), (int64_t)entries[g].size(),
                                entDev + entryBase[g], B, st));
            s->stats[1] += 1;
        }
        MRC_HIP(h, hipEventRecord(b.ev[4], st));
        MRC_HIP(h, launch_band_frames(nSlab, (const BandItem*)(din + oItems), (const long long*)(din + oEdges), n_frames, hop, n_bands,
                                      n_channels_out, format, B, outSlab, st));
        MRC_HIP(h, hipEventRecord(b.ev[5], st));
        MRC_HIP(h, hipStreamSynchronize(st));                // (the staging is written again by the next slab)
        MRC_TRY(add_elapsed(h, b.ev, kSlabSpans, 4, s->ms));
    }
    MRC_HIP(h, hipStreamSynchronize(st));
    return MRC_OK;
}

// the band call's table: int32 [4][MRC_MAX_STORE_BANDS + 1], a shape's line ranges (514 words)
int band_energy_window(mrc_pac_store* s, const FramesRequest& r, int n_bands, const double* edge_hz) {
    constexpr int kRow = MRC_MAX_STORE_BANDS + 1;
    EnergyTable T;
    T.fn = "mrc_pac_store_band_energy_window";
    T.nOut = n_bands;
    T.build = [&](const mrc_config& cfg) {
        T.words.assign((4 * kRow * sizeof(int32_t) + 7) / 8, 0);
        for (int sh = 0; sh < 4; ++sh) {
            int a, b;
            shape_ab(cfg, sh, &a, &b);
            const std::string refusal = band_line_ranges((double)cfg.sample_rate, a, b, n_bands, edge_hz, (int32_t*)T.words.data() + sh * kRow);
            if (!refusal.empty()) return refusal;
        }
        return std::string();
    };
    T.launch = [&](int sh, const DevShape& F, const UnpackGroupDev& G, const int64_t* table, int64_t nEntries,
                   const EnergyEntry* entries, double* sums, hipStream_t st) {
        return launch_band_energy(F, G.joint, n_bands, (const int*)table + sh * kRow, nEntries, entries, G.oscale,
                                  G.joint ? G.ms : nullptr, G.sf, G.ba, G.mant, sums, st);
    };
    return energy_frames_window(s, T, r);
}

// the filter call's table: int32 [4][3][n_filters] (a shape's lo, hi and row offsets, the offsets counted from the shape's
// first weight), then the four shapes' rows of float64 weights one after the other
int filterbank_window(mrc_pac_store* s, const FramesRequest& r, int n_filters, const double* point_hz, int norm) {
    EnergyTable T;
    T.fn = "mrc_pac_store_filterbank_window";
    T.nOut = n_filters;
    size_t rowWord[4] = {0, 0, 0, 0};                        // where a shape's weights start in words
    T.build = [&](const mrc_config& cfg) {
        std::vector<int32_t> lo[4], hi[4];
        std::vector<double> rows[4];
        for (int sh = 0; sh < 4; ++sh) {
            int a, b;
            shape_ab(cfg, sh, &a, &b);
            lo[sh].assign((size_t)std::max(n_filters, 1), 0);
            hi[sh].assign((size_t)std::max(n_filters, 1), 0);
            int64_t n = 0;
            const std::string refusal = filterbank_line_weights(FilterPoints{(double)cfg.sample_rate, n_filters, point_hz, norm}, a, b,
                                                                lo[sh].data(), hi[sh].data(), &rows[sh], &n);
            if (!refusal.empty()) return refusal;
        }
        const size_t nf = (size_t)n_filters;
        size_t at = (12 * nf * sizeof(int32_t) + 7) / 8;
        for (int sh = 0; sh < 4; ++sh) { rowWord[sh] = at; at += rows[sh].size(); }
        T.words.assign(at, 0);
        int32_t* ints = (int32_t*)T.words.data();
        for (int sh = 0; sh < 4; ++sh) {
            int32_t off = 0;
            for (size_t q = 0; q < nf; ++q) {
                ints[(3 * sh + 0) * nf + q] = lo[sh][q];
                ints[(3 * sh + 1) * nf + q] = hi[sh][q];
                ints[(3 * sh + 2) * nf + q] = off;
                off += hi[sh][q] - lo[sh][q];
            }
            if (!rows[sh].empty()) std::memcpy(T.words.data() + rowWord[sh], rows[sh].data(), sizeof(double) * rows[sh].size());
        }
        return std::string();
    };
    T.launch = [&](int sh, const DevShape& F, const UnpackGroupDev& G, const int64_t* table, int64_t nEntries,
                   const EnergyEntry* entries, double* sums, hipStream_t st) {
        return launch_filterbank_energy(F, G.joint, n_filters, (const int*)table + (size_t)3 * sh * n_filters,
                                        (const double*)(table + rowWord[sh]), nEntries, entries, G.oscale, G.joint ? G.ms : nullptr,
                                        G.sf, G.ba, G.mant, sums, st);
    };
    return energy_frames_window(s, T, r);
}

}  // namespace

extern "C" {

int mrc_filterbank_line_weights(double sample_rate, int a, int b, int n_filters, const double* point_hz, int norm,
                                int32_t* line_lo, int32_t* line_hi, int64_t weight_cap, double* weight, int64_t* n_weights) {
    const char* const fn = "mrc_filterbank_line_weights: ";
    std::vector<double> rows;
    const std::string refusal = filterbank_line_weights(FilterPoints{sample_rate, n_filters, point_hz, norm}, a, b, line_lo, line_hi,
                                                        weight ? &rows : nullptr, n_weights);
    if (!refusal.empty()) return fail(nullptr, MRC_ERR_INVALID, fn + refusal);
    if (!weight) return MRC_OK;
    if (weight_cap < (int64_t)rows.size())
        return fail(nullptr, MRC_ERR_INVALID, fn + ("weight_cap " + std::to_string(weight_cap) + " is below the " +
                                                    std::to_string(rows.size()) + " weights of the rows"));
    if (!rows.empty()) std::memcpy(weight, rows.data(), sizeof(double) * rows.size());
    return MRC_OK;
}

int mrc_pac_store_filterbank_window(mrc_pac_store* s, int mix, int64_t n_items, const int64_t* file, const int64_t* start,
                                    int64_t n_frames, int64_t hop, int n_filters, const double* point_hz, int norm,
                                    int n_channels_out, int format, void* out, void* stream) {
    return filterbank_window(s, FramesRequest{mix, n_items, file, start, n_frames, hop, n_channels_out, format, out, stream}, n_filters,
                             point_hz, norm);
}

int mrc_band_line_ranges(double sample_rate, int a, int b, int n_bands, const double* edge_hz, int32_t* line_lo) {
    const std::string refusal = band_line_ranges(sample_rate, a, b, n_bands, edge_hz, line_lo);
    return refusal.empty() ? MRC_OK : fail(nullptr, MRC_ERR_INVALID, "mrc_band_line_ranges: " + refusal);
}

int mrc_pac_store_band_energy_window(mrc_pac_store* s, int mix, int64_t n_items, const int64_t* file, const int64_t* start,
                                     int64_t n_frames, int64_t hop, int n_bands, const double* edge_hz, int n_channels_out,
                                     int format, void* out, void* stream) {
    return band_energy_window(s, FramesRequest{mix, n_items, file, start, n_frames, hop, n_channels_out, format, out, stream}, n_bands,
                              edge_hz);
}

int mrc_resample_taps(int up, int down, int zeros, double rolloff, int32_t* half_width, double* taps) {
    ResampleSpec r;
    const std::string refusal = resample_spec(up, down, zeros, rolloff, &r);
    if (!refusal.empty()) return fail(nullptr, MRC_ERR_INVALID, "mrc_resample_taps: " + refusal);
    if (half_width) *half_width = r.W;
    if (taps) resample_taps(r, taps);
    return MRC_OK;
}

}  // extern "C"

namespace {

// The one check of every window call, made once per public call: every refusal the entries give, under the entry's name and in
// the order each entry has always given them -- the request's own arguments (mix, ratios, rows, bands), the divisor, window,
// channels, format and files, then the bank indices of a reverb or STFT call.  window, format and out are the call's; an STFT
// call passes its row length L (0 without frames) and MRC_WINDOW_F64.  The kinds differ only in where window and out are
// looked at: a reverb call refuses a bad window before its rows and a NULL out last of all, an STFT call has refused its own
// arguments before it comes here and names L in its bound on the pre-roll.
constexpr int64_t kMaxWindow = (int64_t)1 << 40;             // of a window, and of a span's length and |first sample|
int check_windows(mrc_pac_store* s, const WindowRequest& q, int64_t window, int format, void* out, CheckedWindows* c) {
    mrc_handle* h = s->h;
    const std::string w = q.fn;
    const auto refuse = [&](const std::string& what) { return fail(h, MRC_ERR_INVALID, w + ": " + what); };
    const bool rows = q.rows(), banked = q.banked(), routed = q.routed(), stft = q.stft();
    const int C = q.routesPerTerm();
    // a route's place in every refusal that names one
    const auto route = [C](int64_t r) { return "term " + std::to_string(r / C) + ", channel " + std::to_string(r % C); };
    const bool windowOk = window >= 0 && window <= kMaxWindow;
    c->q = q;
    if (q.ratioList && q.nBands == 0 && (q.edgeHz || q.bandGain))
        return refuse("n_bands is 0 (no band gains) but edge_hz or band_gain is not NULL");
    if (banked && !stft && !windowOk) return refuse("window must lie in [0, 2^40]");
    MRC_TRY(check_mix(h, w, q.mix, q.mixAllowed));
    if (routed && (q.routeChannels < 1 || q.routeChannels > MRC_MAX_STORE_ROUTE_CHANNELS))
        return refuse("n_channels_out " + std::to_string(q.routeChannels) + " is outside 1.." + std::to_string(MRC_MAX_STORE_ROUTE_CHANNELS));
    if (q.mix != MRC_MIX_EACH && q.nChannelsOut != 1) return refuse("n_channels_out must be 1 under a mix of one channel");
    c->mix = q.mix == MRC_MIX_EACH ? kNoMix : q.mix;
    // ---- the ratio, or the length of the list
    if (q.ratioList) {
        if (q.nRatios < 1 || q.nRatios > MRC_MAX_STORE_RATIOS)
            return refuse("n_ratios " + std::to_string(q.nRatios) + " is outside 1.." + std::to_string(MRC_MAX_STORE_RATIOS));
    } else if (rows || q.resampled) {
        if (rows && (q.up < 1 || q.down < 1))
            return refuse((q.up < 1 ? "up " + std::to_string(q.up) : "down " + std::to_string(q.down)) + " is below 1");
        if (!rows || q.up != q.down) {                       // (rows at up == down: ratio 1, zeros and rolloff are not looked at)
            const std::string refusal = resample_spec(q.up, q.down, q.zeros, q.rolloff, &c->rs);
            if (!refusal.empty()) return refuse(refusal);
            c->filtered = true;
        }
    }
    // ---- the rows, their terms, the list of ratios and the bands
    if (rows) {
        if (q.nItems < 0) return refuse("n_items < 0");
        if (!q.termOffset) return refuse("term_offset is NULL");
        if (q.termOffset[0] != 0) return refuse("term_offset[0] = " + std::to_string(q.termOffset[0]) + " is not 0");
        for (int64_t i = 0; i < q.nItems; ++i)
            if (q.termOffset[i + 1] < q.termOffset[i]) return refuse("term_offset decreases at [" + std::to_string(i + 1) + "]");
        const int64_t nTerms = c->nTerms = q.termOffset[q.nItems];
        if (routed) {
            if (nTerms > 0 && (!q.file || !q.start)) return refuse("file or start is NULL");
            if (nTerms > 0 && (!q.gain || !q.irOf)) return refuse("route_gain or route_ir is NULL");
            for (int64_t r = 0; r < nTerms * C; ++r)
                if (!std::isfinite(q.gain[r])) return refuse("route_gain of " + route(r) + " is not finite");
        } else {
            if (nTerms > 0 && (!q.file || !q.start || !q.gain)) return refuse("file, start or gain is NULL");
            for (int64_t k = 0; k < nTerms; ++k)
                if (!std::isfinite(q.gain[k])) return refuse("gain of term " + std::to_string(k) + " is not finite");
        }
        if (q.ratioList && nTerms > 0 && (!q.ratioUp || !q.ratioDown || !q.ratioOf))
            return refuse("ratio_up, ratio_down or ratio_of is NULL");
        if (q.ratioList && q.ratioUp && q.ratioDown) {       // the list is checked wherever it is given, terms or none
            c->speeds.nRatios = q.nRatios;
            for (int i = 0; i < q.nRatios; ++i) {
                const int u = q.ratioUp[i], d = q.ratioDown[i];
                const std::string at = "ratio " + std::to_string(i) + ": ";
                if (u < 1 || d < 1) return refuse(at + (u < 1 ? "up " + std::to_string(u) : "down " + std::to_string(d)) + " is not positive");
                c->speeds.r[i] = ResampleSpec{1, 1, 0, 0.0, 0};  // (u == d: the unit ratio, zeros and rolloff are not looked at)
                if (u != d) {
                    const std::string refusal = resample_spec(u, d, q.zeros, q.rolloff, &c->speeds.r[i]);
                    if (!refusal.empty()) return refuse(at + refusal);
                }
            }
            for (int64_t k = 0; k < nTerms; ++k)             // (terms present: ratio_of is not NULL)
                if (q.ratioOf[k] < 0 || q.ratioOf[k] >= q.nRatios)
                    return refuse("ratio_of of term " + std::to_string(k) + " = " + std::to_string(q.ratioOf[k]) +
                                  " is outside the list of " + std::to_string(q.nRatios) + " ratios");
        }
        c->speedy = q.ratioList && nTerms > 0;
        if (q.banded) {
            const int nb = q.nBands;
            if (nb < 1 || nb > MRC_MAX_STORE_BANDS)
                return refuse("n_bands " + std::to_string(nb) + " is outside 1.." + std::to_string(MRC_MAX_STORE_BANDS));
            if (nTerms > 0 && (!q.edgeHz || !q.bandGain)) return refuse("edge_hz or band_gain is NULL");
            int32_t lineLo[MRC_MAX_STORE_BANDS + 1];
            for (int sh = 0; q.edgeHz && sh < 4; ++sh) {     // per call one uint16 line-to-band table per block shape
                int a, b;
                shape_ab(h->cfg, sh, &a, &b);
                const std::string refusal = band_line_ranges((double)h->cfg.sample_rate, a, b, nb, q.edgeHz, lineLo);
                if (!refusal.empty()) return refuse(refusal);
                c->shape.lineOff[sh] = (int64_t)c->shape.lineBand.size();
                c->shape.lineBand.resize(c->shape.lineBand.size() + (size_t)((a + b) / 2), kNoLineBand);
                uint16_t* lb = c->shape.lineBand.data() + c->shape.lineOff[sh];
                for (int b0 = 0; b0 < nb; ++b0)
                    for (int k = lineLo[b0]; k < lineLo[b0 + 1]; ++k) lb[k] = (uint16_t)b0;
            }
            for (int64_t k = 0; k < nTerms; ++k)
                for (int b0 = 0; b0 < nb; ++b0)
                    if (!std::isfinite(q.bandGain[k * nb + b0]))
                        return refuse("band_gain of term " + std::to_string(k) + ", band " + std::to_string(b0) + " is not finite");
            c->shaped = true;
        }
        // ---- the spans and their fades
        if ((q.spanFirst != nullptr) != (q.spanLen != nullptr))
            return refuse(q.spanFirst ? "span_first is given without span_len" : "span_len is given without span_first");
        if (!q.spanFirst && (q.fadeIn || q.fadeOut))
            return refuse(std::string(q.fadeIn ? "fade_in" : "fade_out") + " is given without spans (span_first and span_len)");
        for (int64_t k = 0; q.spanFirst && k < nTerms; ++k) {
            const std::string term = " of term " + std::to_string(k);
            const int64_t len = q.spanLen[k], first = q.spanFirst[k], fi = q.fadeIn ? q.fadeIn[k] : 0, fo = q.fadeOut ? q.fadeOut[k] : 0;
            if (len < 0 || len > kMaxWindow) return refuse("span_len" + term + " = " + std::to_string(len) + " is outside [0, 2^40]");
            if (first < -kMaxWindow || first > kMaxWindow)
                return refuse("span_first" + term + " = " + std::to_string(first) + " is outside [-2^40, 2^40]");
            if (fi < 0) return refuse("fade_in" + term + " = " + std::to_string(fi) + " is negative");
            if (fo < 0) return refuse("fade_out" + term + " = " + std::to_string(fo) + " is negative");
            if (fi > len || fo > len - fi)
                return refuse("fade_in + fade_out" + term + " = " + std::to_string(fi) + " + " + std::to_string(fo) +
                              " exceeds its span_len = " + std::to_string(len));
        }
    }
    // ---- what every window call is asked: divisor, window, channels, format, files
    MRC_TRY(check_divisor(h, w, q.rateDivisor));
    if (!rows) {
        if (q.nItems < 0) return refuse("n_items < 0");
        c->nTerms = q.nItems;
    }
    if (!windowOk) return refuse("window must lie in [0, 2^40]");
    if (q.nChannelsOut != 1 && q.nChannelsOut != 2) return refuse("n_channels_out must be 1 or 2");
    if (format != MRC_WINDOW_PCM16 && format != MRC_WINDOW_F32 && format != MRC_WINDOW_F64)
        return refuse("unknown format " + std::to_string(format));
    if (!rows && q.nItems > 0 && (!q.file || !q.start)) return refuse("file or start is NULL");
    c->empty = q.nItems == 0 || window == 0;
    if (!banked && !c->empty && !out) return refuse("out is NULL");
    MRC_TRY(check_files(s, w, c->nTerms, q.file, c->mix == kNoMix ? q.nChannelsOut : 0, rows ? "term" : "item"));
    if (!banked) return MRC_OK;
    // ---- the terms' impulse responses
    const int64_t nIrs = (int64_t)s->irLen.size();
    if (c->nTerms > 0 && !q.irOf) return refuse("ir_of is NULL");
    for (int64_t r = 0; r < c->nTerms * C; ++r) {
        const int64_t v = q.irOf[r];
        if (v == -1 || (routed && v == MRC_ROUTE_NONE)) continue;
        const std::string name = routed ? "route_ir of " + route(r) : "ir_of of term " + std::to_string(r);
        if (v >= 0 && nIrs == 0)
            return refuse(name + " = " + std::to_string(v) + " but the store has no impulse responses (mrc_pac_store_set_irs)");
        if (v < 0 || v >= nIrs)
            return refuse(name + " = " + std::to_string(v) + (routed ? " is none of MRC_ROUTE_NONE (-2), -1 and an index into the bank of " :
                                                                       " is neither -1 nor inside the bank of ") +
                          std::to_string(nIrs) + " impulse responses");
        c->maxPreRoll = std::max(c->maxPreRoll, s->irLen[(size_t)v] - 1);
    }
    const std::string tooLong = " + the longest impulse response named - 1 = " + std::to_string(window + c->maxPreRoll) + " exceeds 2^40";
    const bool overlong = window + c->maxPreRoll > kMaxWindow;
    if (!stft && overlong) return refuse("window" + tooLong);
    if (!c->empty && !out) return refuse("out is NULL");
    if (stft && !c->empty && overlong) return refuse("L" + tooLong);
    return MRC_OK;
}

// The reverb loop: per slab of whole rows the units loop decodes every term as a row of its own at gain 1.0 over
// (start - Lpre, window + Lpre) in MRC_WINDOW_F64 into StoreBufs::reverbDry, then reverb_forward_kernel transforms the
// convolved terms' segments and reverb_fold_kernel folds the rows (mrc_kernels_reverb.hip), on the same stream.  The term and
// source records of a slab go up in one copy.
const char* const kWinReverb = "mrc_pac_store_decode_window_reverb";
const char* const kWinRouted = "mrc_pac_store_decode_window_routed";
const char* const kWinSpans = "mrc_pac_store_decode_window_spans";
const char* const kSetIrs = "mrc_pac_store_set_irs";
constexpr int64_t kRevB = MRC_STORE_REVERB_BLOCK, kRevN = 2 * kRevB;

// the first quadrant of exp(-2 pi i t / N), rounded from long double, on the device once per handle
int ensure_reverb_twiddles(mrc_handle* h) {
    StoreBufs& b = h->store;
    if (b.reverbTw.p) return MRC_OK;
    std::vector<double2> w((size_t)(kRevN / 4));
    const long double step = 2.0L * acosl(-1.0L) / (long double)kRevN;
    for (int64_t t = 0; t < kRevN / 4; ++t) w[(size_t)t] = make_double2((double)cosl(step * t), (double)-sinl(step * t));
    DevBuf tw;
    MRC_HIP(h, tw.reserve(sizeof(double2) * w.size()));
    MRC_HIP(h, hipMemcpy(tw.p, w.data(), sizeof(double2) * w.size(), hipMemcpyHostToDevice));
    b.reverbTw = std::move(tw);
    return MRC_OK;
}

int set_irs(mrc_pac_store* s, int64_t n_irs, const int64_t* ir_offset, const double* taps) {
    MRC_TRY(store_alive(s, kSetIrs));
    mrc_handle* h = s->h;
    const std::string w = kSetIrs;
    if (n_irs < 0) return fail(h, MRC_ERR_INVALID, w + ": n_irs < 0");
    if (n_irs > 0 && (!ir_offset || !taps)) return fail(h, MRC_ERR_INVALID, w + ": ir_offset or taps is NULL");
    if (n_irs > 0 && ir_offset[0] != 0) return fail(h, MRC_ERR_INVALID, w + ": ir_offset[0] = " + std::to_string(ir_offset[0]) + " is not 0");
    for (int64_t j = 0; j < n_irs; ++j) {
        const int64_t len = ir_offset[j + 1] - ir_offset[j];
        if (len < 1 || len > MRC_MAX_STORE_IR_TAPS)
            return fail(h, MRC_ERR_INVALID, w + ": impulse response " + std::to_string(j) + " has " + std::to_string(len) +
                                                " taps, outside 1.." + std::to_string(MRC_MAX_STORE_IR_TAPS));
    }
    for (int64_t j = 0; j < n_irs; ++j)
        for (int64_t i = ir_offset[j]; i < ir_offset[j + 1]; ++i)
            if (!std::isfinite(taps[i]))
                return fail(h, MRC_ERR_INVALID, w + ": taps[" + std::to_string(i) + "] (impulse response " + std::to_string(j) + ") is not finite");
    MRC_HIP(h, hipSetDevice(h->device));
    hipStream_t st = pick_stream(h, nullptr);
    MRC_HIP(h, hipStreamSynchronize(st));
    s->irBank = DevBuf();                                    // the call replaces the bank; a failure below leaves none
    s->irLen.clear();
    s->irPart.clear();
    if (n_irs == 0) return MRC_OK;

    std::vector<int64_t> len((size_t)n_irs), part((size_t)n_irs);
    std::vector<ReverbSource> src((size_t)n_irs);
    int64_t nPart = 0, maxSeg = 0;
    for (int64_t j = 0; j < n_irs; ++j) {
        len[(size_t)j] = ir_offset[j + 1] - ir_offset[j];
        part[(size_t)j] = nPart;
        const int64_t P = (len[(size_t)j] + kRevB - 1) / kRevB;
        src[(size_t)j] = ReverbSource{ir_offset[j], -1, 0, 0, len[(size_t)j], nPart, (int)P, (int)kRevB};
        nPart += P;
        maxSeg = std::max(maxSeg, P);
    }
    const size_t nTaps = (size_t)ir_offset[n_irs];
    DevBuf bank, tapsDev, srcDev;
    for (auto need : {std::make_pair(&bank, sizeof(double2) * (size_t)(nPart * kRevN)), std::make_pair(&tapsDev, sizeof(double) * nTaps),
                      std::make_pair(&srcDev, sizeof(ReverbSource) * src.size())})
        if (need.first->reserve(need.second) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, MRC_ERR_NOMEM, w + ": out of device memory for " + std::to_string(nPart) + " partitions of " +
                                              std::to_string(kRevN) + " bins; the store has no impulse responses now");
        }
    MRC_TRY(ensure_reverb_twiddles(h));
    MRC_HIP(h, hipMemcpy(tapsDev.p, taps, sizeof(double) * nTaps, hipMemcpyHostToDevice));
    MRC_HIP(h, hipMemcpy(srcDev.p, src.data(), sizeof(ReverbSource) * src.size(), hipMemcpyHostToDevice));
    MRC_HIP(h, launch_reverb_forward(n_irs, maxSeg, srcDev.as<ReverbSource>(), tapsDev.as<double>(), h->store.reverbTw.as<double2>(),
                                     bank.as<double2>(), st));
    MRC_HIP(h, hipStreamSynchronize(st));
    s->irBank = std::move(bank);
    s->irLen = std::move(len);
    s->irPart = std::move(part);
    return MRC_OK;
}

// Two things follow from the RANGE the loop is given -- the whole call from decode_window_reverb, one STFT slab from
// stft_loop -- and are kept as the nesting of the entries once made them:
//   Lpre, the pre-roll, is the longest response named by the terms of the range - 1, not of the call: it decides which
//   blocks are decoded and so chunks_parsed;
//   a range without a convolved term takes the plain rows path: no dry buffer, no fold, the units loop's own slabs.
constexpr int kReverbSpans[2][2] = {{0, 1}, {1, 2}};         // StoreBufs::reverbEv: forward | fold
int reverb_loop(mrc_pac_store* s, const CheckedWindows& c, const WindowRun& run) {
    const WindowRequest& q = c.q;
    mrc_handle* h = s->h;
    const int64_t* const term_offset = q.termOffset;
    const int32_t* const ir_of = q.irOf;
    // A routed request is the same loop with C routes per term where the others have one: gain and ir_of are [term][C], the
    // terms are decoded with ONE channel, the rows have C, a term has a source per distinct response LENGTH among its wet
    // routes (spectra are shared exactly where the lengths are equal: a segment is zero outside [-(len(h) - 1), window) and
    // the number of segments follows len(h)), and reverb_route_fold_kernel folds.  A range without a wet route takes the
    // plain rows path only where that IS the row: one channel, no absent route (gain is then the rows call's [n_terms]).
    const bool routed = q.routed();
    const int C = q.routesPerTerm(), nch = q.nChannelsOut, nchOut = q.rowChannels();
    int64_t Lpre = 0;
    bool absent = false;
    for (int64_t r = term_offset[run.first] * C; r < term_offset[run.last] * C; ++r) {
        if (ir_of[r] >= 0) Lpre = std::max(Lpre, s->irLen[(size_t)ir_of[r]]);     // (longest length; at least 1 if any)
        absent = absent || ir_of[r] == MRC_ROUTE_NONE;
    }
    if (Lpre == 0 && (!routed || (C == 1 && !absent))) return units_loop(s, c, run);
    Lpre = std::max<int64_t>(Lpre, 1) - 1;
    const int64_t window = run.window, Wd = window + Lpre;
    const int format = run.format;
    // the distinct response lengths among term k's wet routes, in the order of their first channel -> their number
    const auto lengths_of = [&](int64_t k, int64_t* lens) {
        int n = 0;
        for (int ch = 0; ch < C; ++ch) {
            const int64_t v = ir_of[k * C + ch];
            if (v < 0) continue;
            const int64_t len = s->irLen[(size_t)v];
            if (std::find(lens, lens + n, len) == lens + n) lens[n++] = len;
        }
        return n;
    };

    MRC_HIP(h, hipSetDevice(h->device));
    MRC_TRY(ensure_reverb_twiddles(h));
    StoreBufs& b = h->store;
    MRC_HIP(h, b.reverbEv.create());
    hipStream_t st = pick_stream(h, q.stream);
    DrainGuard drain{{st, nullptr, nullptr}};
    const size_t elem = format == MRC_WINDOW_PCM16 ? 2 : format == MRC_WINDOW_F32 ? 4 : 8;
    // (a row takes M workgroups, a routed row at most M per channel: the fold's grid stays below 2^31)
    const int64_t M = (window + kRevB - 1) / kRevB, slab = run.slab, rowCap = std::max<int64_t>(1, 0x7fffffffLL / (M * C));
    for (int64_t first = run.first, last; first < run.last; first = last) {   // rows [first, last), their terms [u0, u0 + nT)
        last = first + 1;
        while (last < run.last && last - first < rowCap && (slab == 0 || (term_offset[last + 1] - term_offset[first]) * Wd <= slab)) ++last;
        const int64_t nRows = last - first, u0 = term_offset[first], nT = term_offset[last] - u0;
        unsigned char* outSlab = (unsigned char*)run.out + (size_t)(first - run.first) * nchOut * window * elem;
        if (nT == 0) {                                       // rows without terms: +0.0
            MRC_HIP(h, hipMemsetAsync(outSlab, 0, (size_t)nRows * nchOut * window * elem, st));
            s->stats[2] += 1;
            continue;
        }
        // ---- the dry terms, by the units loop.  The slab is cut here, by output samples: the units loop runs it as one and
        // does not cut it again by its intermediate spans, which would leave a short second slab behind every full one
        MRC_HIP(h, b.reverbDry.reserve(sizeof(double) * (size_t)(nT * nch * Wd)));
        MRC_TRY(units_loop(s, c, WindowRun{u0, u0 + nT, Wd, MRC_WINDOW_F64, b.reverbDry.p, 0, Lpre, true}));

        // ---- the records (one H2D copy): terms, C routes each | the rows' term offsets | sources
        int64_t nConv = 0, nSpec = 0, maxSeg = 0, lens[MRC_MAX_STORE_ROUTE_CHANNELS], specOf[MRC_MAX_STORE_ROUTE_CHANNELS];
        for (int64_t k = 0; k < nT; ++k)
            for (int i = 0, n = lengths_of(u0 + k, lens); i < n; ++i) {
                const int64_t nSeg = M + (lens[i] + kRevB - 1) / kRevB - 1;
                nConv += 1;
                nSpec += nSeg;
                maxSeg = std::max(maxSeg, nSeg);
            }
        StageLayout lay(256);
        const size_t oTerms = lay.add<ReverbTerm>(nT * C), oRows = lay.add<long long>(nRows + 1), oSrc = lay.add<ReverbSource>(nConv);
        MRC_HIP(h, b.reverbPin.reserve(lay.total()));
        MRC_HIP(h, b.reverbIn.reserve(lay.total()));
        MRC_HIP(h, b.reverbSpec.reserve(std::max<size_t>(sizeof(double2) * (size_t)(nSpec * kRevN), 256)));
        unsigned char* pin = (unsigned char*)b.reverbPin.p;
        ReverbTerm* terms = (ReverbTerm*)(pin + oTerms);
        long long* rowTerms = (long long*)(pin + oRows);
        ReverbSource* src = (ReverbSource*)(pin + oSrc);
        for (int64_t r = 0; r <= nRows; ++r) rowTerms[r] = term_offset[first + r] - u0;
        int64_t nWet = 0, nPaired = 0;                       // wet routes | those whose neighbour in a group of two shares their source
        for (int64_t k = 0, conv = 0, spec = 0; k < nT; ++k) {
            const int64_t base = k * nch * Wd;
            const int n = lengths_of(u0 + k, lens);
            for (int i = 0; i < n; ++i) {
                const int64_t P = (lens[i] + kRevB - 1) / kRevB, nSeg = M + P - 1;
                specOf[i] = spec;
                src[conv++] = ReverbSource{base, nch == 2 ? base + Wd : -1, Lpre - P * kRevB, Lpre - (lens[i] - 1), Wd, spec, (int)nSeg, (int)kRevN};
                spec += nSeg;
            }
            for (int ch = 0; ch < C; ++ch) {
                const int64_t r = (u0 + k) * C + ch, v = ir_of[r];
                if (v < 0) {                                 // -1 dry (kRouteDry), MRC_ROUTE_NONE absent (kRouteNone)
                    terms[k * C + ch] = ReverbTerm{base + Lpre, v, 0, 0, 0, q.gain[r]};
                    continue;
                }
                const int64_t len = s->irLen[(size_t)v];
                terms[k * C + ch] = ReverbTerm{base + Lpre, specOf[std::find(lens, lens + n, len) - lens], s->irPart[(size_t)v],
                                               (int)((len + kRevB - 1) / kRevB), 0, q.gain[r]};
                nWet += 1;
                if (ch & 1) nPaired += 2 * (terms[k * C + ch - 1].spec == terms[k * C + ch].spec);
            }
        }
        // the channels one workgroup serves: two where at least half the slab's wet routes then load their spectra together
        // (an array's microphones), else one -- measured; the option forces either, the bits are the same
        const int group = h->storeRouteGroup ? h->storeRouteGroup : 2 * nPaired >= nWet && nWet > 0 ? 2 : 1;
        if (routed) {
            s->routeInfo[0] += nSpec;
            s->routeInfo[1] += nWet * M;
            s->routeInfo[2] += nSpec * kRevN * (int64_t)sizeof(double2);
        }
        // ---- device: forward transforms of the convolved terms' segments, then the rows
        unsigned char* din = b.reverbIn.as<unsigned char>();
        MRC_HIP(h, hipMemcpyAsync(din, pin, lay.total(), hipMemcpyHostToDevice, st));
        MRC_HIP(h, hipEventRecord(b.reverbEv[0], st));
        MRC_HIP(h, launch_reverb_forward(nConv, maxSeg, (const ReverbSource*)(din + oSrc), b.reverbDry.as<double>(),
                                         b.reverbTw.as<double2>(), b.reverbSpec.as<double2>(), st));
        MRC_HIP(h, hipEventRecord(b.reverbEv[1], st));
        if (routed)
            MRC_HIP(h, launch_reverb_route_fold(nRows, (const ReverbTerm*)(din + oTerms), (const long long*)(din + oRows), window, C,
                                                group, format, b.reverbDry.as<double>(), b.reverbSpec.as<double2>(),
                                                s->irBank.as<double2>(), b.reverbTw.as<double2>(), outSlab, st));
        else
            MRC_HIP(h, launch_reverb_fold(nRows, (const ReverbTerm*)(din + oTerms), (const long long*)(din + oRows), window, nch, format,
                                          Wd, b.reverbDry.as<double>(), b.reverbSpec.as<double2>(), s->irBank.as<double2>(),
                                          b.reverbTw.as<double2>(), outSlab, st));
        MRC_HIP(h, hipEventRecord(b.reverbEv[2], st));
        MRC_HIP(h, hipStreamSynchronize(st));                // (the staging is written again by the next slab)
        MRC_TRY(add_elapsed(h, b.reverbEv, kReverbSpans, 2, s->reverbMs));
    }
    MRC_HIP(h, hipStreamSynchronize(st));
    return MRC_OK;
}

// A window call from its request to its statistics: the totals zeroed, the one check, the loop of the request's kind over all
// its rows under the handle's slab limit, and the reverb kernels' time counted into ms[3] once.
int window_call(mrc_pac_store* s, const WindowRequest& q, int64_t window, int format, void* out) {
    MRC_TRY(store_alive(s, q.fn));
    const bool reverb = q.banked();
    reset_stats(s);
    if (reverb) s->reverbMs[0] = s->reverbMs[1] = 0.0;
    if (q.routed()) s->routeInfo[0] = s->routeInfo[1] = s->routeInfo[2] = 0;
    CheckedWindows c;
    MRC_TRY(check_windows(s, q, window, format, out, &c));
    if (c.empty) return MRC_OK;
    const WindowRun all{0, q.nItems, window, format, out, s->h->storeSlabSamples};
    MRC_TRY(reverb ? reverb_loop(s, c, all) : units_loop(s, c, all));
    if (reverb) s->ms[3] += s->reverbMs[0] + s->reverbMs[1];
    return MRC_OK;
}

// The STFT loop: per slab of whole rows the reverb loop writes the rows as MRC_WINDOW_F64 over L = (n_frames - 1) hop + n_fft
// samples into StoreBufs::stftRows (its own dry-term scratch is in use underneath), then stft_kernel (mrc_kernels_stft.hip)
// frames and transforms them on the same stream.  The twiddles, the frame window and the bank's supports and weights go up once
// per call.
const char* const kStft = "mrc_pac_store_stft_window";
const char* const kStftRouted = "mrc_pac_store_stft_window_routed";
const char* const kStftWithSpans = "mrc_pac_store_stft_window_spans";

// exp(-2 pi i t / n) for 0 <= t < n from long double, the quadrant taken out first: the axes are exact
void stft_twiddles(int n, double2* w) {
    const long double halfPi = acosl(-1.0L) / 2.0L;
    for (int t = 0; t < n; ++t) {
        const int q = (int)((4LL * t) / n);
        const long double th = halfPi * (long double)(4LL * t - (long long)q * n) / (long double)n;
        const double c = (double)cosl(th), sn = (double)sinl(th);
        w[t] = q == 0 ? make_double2(c, -sn) : q == 1 ? make_double2(-sn, -c) : q == 2 ? make_double2(-c, sn) : make_double2(sn, c);
    }
}

// rows [run.first, run.last) of the checked request through stft_kernel: P holds the call's tables and sizes, run.window is
// P.L and run.out the first row's output
constexpr int kStftSpans[1][2] = {{0, 1}};                   // StoreBufs::stftEv: stft_kernel
int stft_loop(mrc_pac_store* s, const CheckedWindows& c, StftParams P, const WindowRun& run) {
    mrc_handle* h = s->h;
    StoreBufs& b = h->store;
    MRC_HIP(h, b.stftEv.create());
    hipStream_t st = pick_stream(h, c.q.stream);
    DrainGuard drain{{st, nullptr, nullptr}};
    const int nch = P.nch;
    const int64_t L = run.window, nOut = P.mode == MRC_STFT_BANK ? P.nFilters : P.nFft / 2 + 1;
    const size_t rowBytes = (size_t)nch * (size_t)nOut * (size_t)P.nFrames * (P.format == MRC_WINDOW_F32 ? 4 : 8) * (P.mode == MRC_STFT_COMPLEX ? 2 : 1);
    const int64_t slab = run.slab, rowCap = std::max<int64_t>(1, 0x7fffffffLL / (nch * P.nFrames));
    for (int64_t first = run.first, last; first < run.last; first = last) {   // rows [first, last)
        last = first + 1;
        while (last < run.last && last - first < rowCap && (slab == 0 || (last + 1 - first) * L <= slab)) ++last;
        const int64_t nRows = last - first;
        MRC_HIP(h, b.stftRows.reserve(sizeof(double) * (size_t)(nRows * nch * L)));
        // (the slab is cut here, by the rows' samples: the reverb loop runs it as one slab of its own)
        MRC_TRY(reverb_loop(s, c, WindowRun{first, last, L, MRC_WINDOW_F64, b.stftRows.p, 0}));
        P.rows = b.stftRows.as<double>();
        P.out = (unsigned char*)run.out + (size_t)(first - run.first) * rowBytes;
        P.nRows = (int)nRows;
        MRC_HIP(h, hipEventRecord(b.stftEv[0], st));
        MRC_HIP(h, launch_stft(P, st));
        MRC_HIP(h, hipEventRecord(b.stftEv[1], st));
        MRC_HIP(h, hipStreamSynchronize(st));
        MRC_TRY(add_elapsed(h, b.stftEv, kStftSpans, 1, &s->stftMs));
    }
    return MRC_OK;
}

struct StftArgs {                                            // the entry's own arguments, as the header names them
    int n_fft;
    const double* frame_window;
    int64_t n_frames, hop;
    int mode, n_filters;
    const double* bank;
};
// mrc_pac_store_stft_window from its request: the call's own arguments are refused first, then the request's (check_windows);
// the tables go up, the loop runs over all rows under the handle's slab limit, stft_kernel's time is counted into ms[3] once
int stft_call(mrc_pac_store* s, const WindowRequest& q, const StftArgs& a, int format, void* out) {
    const char* const fn = q.fn;
    MRC_TRY(store_alive(s, fn));
    mrc_handle* h = s->h;
    const std::string w = fn;
    const int n_fft = a.n_fft, mode = a.mode, n_filters = a.n_filters, n_channels_out = q.rowChannels();
    const int64_t n_frames = a.n_frames, hop = a.hop;
    const double *const frame_window = a.frame_window, *const bank = a.bank;
    reset_stats(s);
    s->stftMs = s->reverbMs[0] = s->reverbMs[1] = 0.0;
    if (q.routed()) s->routeInfo[0] = s->routeInfo[1] = s->routeInfo[2] = 0;
    // ---- this call's own arguments
    int nRad = 0;
    if (n_fft < 16 || n_fft > MRC_MAX_STFT_POINTS || (n_fft & 1) || stft_radices(n_fft / 2, &nRad) == 0)
        return fail(h, MRC_ERR_INVALID, w + ": n_fft " + std::to_string(n_fft) + " must be even, in 16.." +
                                            std::to_string(MRC_MAX_STFT_POINTS) + " and a product of 2s, 3s and 5s");
    const unsigned long long radices = stft_radices(n_fft / 2, &nRad);
    if (!frame_window) return fail(h, MRC_ERR_INVALID, w + ": frame_window is NULL");
    for (int i = 0; i < n_fft; ++i)
        if (!std::isfinite(frame_window[i])) return fail(h, MRC_ERR_INVALID, w + ": frame_window[" + std::to_string(i) + "] is not finite");
    if (n_frames < 0) return fail(h, MRC_ERR_INVALID, w + ": n_frames < 0");
    if (hop < 1) return fail(h, MRC_ERR_INVALID, w + ": hop < 1");
    const int64_t kMaxL = (int64_t)1 << 40;
    if (n_frames > 0 && (hop > kMaxL || n_frames - 1 > (kMaxL - n_fft) / hop))
        return fail(h, MRC_ERR_INVALID, w + ": L = (n_frames - 1) hop + n_fft exceeds 2^40");
    if (mode != MRC_STFT_COMPLEX && mode != MRC_STFT_POWER && mode != MRC_STFT_BANK)
        return fail(h, MRC_ERR_INVALID, w + ": mode " + std::to_string(mode) + " is none of MRC_STFT_COMPLEX, _POWER, _BANK");
    if (format != MRC_WINDOW_F32 && format != MRC_WINDOW_F64)
        return fail(h, MRC_ERR_INVALID, w + ": format " + std::to_string(format) + " is neither MRC_WINDOW_F32 nor MRC_WINDOW_F64");
    const int nBins = n_fft / 2 + 1;
    if (mode == MRC_STFT_BANK) {
        if (n_filters < 1 || n_filters > MRC_MAX_STORE_BANDS)
            return fail(h, MRC_ERR_INVALID, w + ": n_filters " + std::to_string(n_filters) + " outside 1.." + std::to_string(MRC_MAX_STORE_BANDS));
        if (!bank) return fail(h, MRC_ERR_INVALID, w + ": bank is NULL");
        for (int64_t i = 0; i < (int64_t)n_filters * nBins; ++i)
            if (!std::isfinite(bank[i]))
                return fail(h, MRC_ERR_INVALID, w + ": bank[" + std::to_string(i / nBins) + "][" + std::to_string(i % nBins) + "] is not finite");
    } else if (n_filters != 0 || bank) {
        return fail(h, MRC_ERR_INVALID, w + ": n_filters must be 0 and bank NULL unless mode is MRC_STFT_BANK");
    }
    // ---- the request's, with the rows' length L as its window
    const int64_t L = n_frames == 0 ? 0 : (n_frames - 1) * hop + n_fft;
    CheckedWindows c;
    MRC_TRY(check_windows(s, q, L, MRC_WINDOW_F64, out, &c));
    if (c.empty) return MRC_OK;

    MRC_HIP(h, hipSetDevice(h->device));
    StoreBufs& b = h->store;
    hipStream_t st = pick_stream(h, q.stream);
    // ---- the tables (one copy): twiddles | frame window | weights on the supports | lo, hi, offset per filter
    const int nF = mode == MRC_STFT_BANK ? n_filters : 0;
    std::vector<int32_t> tab((size_t)(3 * nF));
    std::vector<double> weights;
    for (int f = 0; f < nF; ++f) {
        const double* row = bank + (size_t)f * nBins;
        int lo = 0, hi = nBins;
        while (lo < nBins && row[lo] == 0.0) ++lo;
        while (hi > lo && row[hi - 1] == 0.0) --hi;
        if (lo == nBins) lo = hi = 0;
        tab[(size_t)f] = lo;
        tab[(size_t)(nF + f)] = hi;
        tab[(size_t)(2 * nF + f)] = (int32_t)weights.size();
        weights.insert(weights.end(), row + lo, row + hi);
    }
    StageLayout lay(256);
    const size_t oTw = lay.add<double2>(n_fft), oWin = lay.add<double>(n_fft), oW = lay.add<double>((int64_t)weights.size()),
                 oTab = lay.add<int32_t>((int64_t)tab.size());
    std::vector<unsigned char> host(lay.total());
    stft_twiddles(n_fft, (double2*)(host.data() + oTw));
    memcpy(host.data() + oWin, frame_window, sizeof(double) * (size_t)n_fft);
    if (!weights.empty()) memcpy(host.data() + oW, weights.data(), sizeof(double) * weights.size());
    if (!tab.empty()) memcpy(host.data() + oTab, tab.data(), sizeof(int32_t) * tab.size());
    MRC_HIP(h, hipStreamSynchronize(st));                    // (an earlier call's kernel may still read the tables)
    MRC_HIP(h, b.stftTab.reserve(lay.total()));
    MRC_HIP(h, hipMemcpy(b.stftTab.p, host.data(), lay.total(), hipMemcpyHostToDevice));
    const unsigned char* dtab = b.stftTab.as<unsigned char>();

    StftParams P{};
    P.win = (const double*)(dtab + oWin);
    P.tw = (const double2*)(dtab + oTw);
    P.bankTab = (const int*)(dtab + oTab);
    P.bankW = (const double*)(dtab + oW);
    P.L = L; P.nFrames = n_frames; P.hop = hop; P.radices = radices;
    P.nch = n_channels_out; P.nFft = n_fft; P.nRad = nRad; P.mode = mode; P.format = format; P.nFilters = nF;
    MRC_TRY(stft_loop(s, c, P, WindowRun{0, q.nItems, L, format, out, h->storeSlabSamples}));
    s->ms[3] += s->reverbMs[0] + s->reverbMs[1] + s->stftMs;
    return MRC_OK;
}

}  // namespace

extern "C" {

int mrc_pac_store_set_irs(mrc_pac_store* s, int64_t n_irs, const int64_t* ir_offset, const double* taps) {
    return set_irs(s, n_irs, ir_offset, taps);
}

int mrc_pac_store_ir_info(mrc_pac_store* s, int64_t* n_irs, int64_t* ir_len) {
    MRC_TRY(store_alive(s, "mrc_pac_store_ir_info"));
    if (n_irs) *n_irs = (int64_t)s->irLen.size();
    for (size_t j = 0; ir_len && j < s->irLen.size(); ++j) ir_len[j] = s->irLen[j];
    return MRC_OK;
}

int mrc_pac_store_decode_window_reverb(mrc_pac_store* s, int rate_divisor, int mix, int n_ratios, const int32_t* ratio_up,
                                       const int32_t* ratio_down, int zeros, double rolloff, int n_bands, const double* edge_hz,
                                       const double* band_gain, int64_t n_items, const int64_t* term_offset, const int64_t* file,
                                       const int64_t* start, const double* gain, const int32_t* ratio_of, const int32_t* ir_of,
                                       int64_t window, int n_channels_out, int format, void* out, void* stream) {
    WindowRequest q{kWinReverb, WindowRequest::kReverb};
    q.rateDivisor = rate_divisor; q.mix = mix; q.zeros = zeros; q.rolloff = rolloff;
    q.ratioList = true; q.nRatios = n_ratios; q.ratioUp = ratio_up; q.ratioDown = ratio_down; q.ratioOf = ratio_of;
    q.banded = n_bands != 0; q.nBands = n_bands; q.edgeHz = edge_hz; q.bandGain = band_gain;
    q.nItems = n_items; q.termOffset = term_offset; q.file = file; q.start = start; q.gain = gain; q.irOf = ir_of;
    q.nChannelsOut = n_channels_out; q.stream = stream;
    return window_call(s, q, window, format, out);
}

int mrc_pac_store_decode_window_spans(mrc_pac_store* s, int rate_divisor, int mix, int n_ratios, const int32_t* ratio_up,
                                      const int32_t* ratio_down, int zeros, double rolloff, int n_bands, const double* edge_hz,
                                      const double* band_gain, int64_t n_items, const int64_t* term_offset, const int64_t* file,
                                      const int64_t* start, const double* gain, const int32_t* ratio_of, const int32_t* ir_of,
                                      const int64_t* span_first, const int64_t* span_len, const int64_t* fade_in,
                                      const int64_t* fade_out, int64_t window, int n_channels_out, int format, void* out,
                                      void* stream) {
    WindowRequest q{kWinSpans, WindowRequest::kReverb};
    q.rateDivisor = rate_divisor; q.mix = mix; q.zeros = zeros; q.rolloff = rolloff;
    q.ratioList = true; q.nRatios = n_ratios; q.ratioUp = ratio_up; q.ratioDown = ratio_down; q.ratioOf = ratio_of;
    q.banded = n_bands != 0; q.nBands = n_bands; q.edgeHz = edge_hz; q.bandGain = band_gain;
    q.nItems = n_items; q.termOffset = term_offset; q.file = file; q.start = start; q.gain = gain; q.irOf = ir_of;
    q.spanFirst = span_first; q.spanLen = span_len; q.fadeIn = fade_in; q.fadeOut = fade_out;
    q.nChannelsOut = n_channels_out; q.stream = stream;
    return window_call(s, q, window, format, out);
}

int mrc_pac_store_stft_window_spans(mrc_pac_store* s, int rate_divisor, int mix, int n_ratios, const int32_t* ratio_up,
                                    const int32_t* ratio_down, int zeros, double rolloff, int n_bands, const double* edge_hz,
                                    const double* band_gain, int64_t n_items, const int64_t* term_offset, const int64_t* file,
                                    const int64_t* start, const double* gain, const int32_t* ratio_of, const int32_t* ir_of,
                                    const int64_t* span_first, const int64_t* span_len, const int64_t* fade_in,
                                    const int64_t* fade_out, int n_fft, const double* frame_window, int64_t n_frames, int64_t hop,
                                    int mode, int n_filters, const double* bank, int n_channels_out, int format, void* out,
                                    void* stream) {
    WindowRequest q{kStftWithSpans, WindowRequest::kStft};
    q.rateDivisor = rate_divisor; q.mix = mix; q.zeros = zeros; q.rolloff = rolloff;
    q.ratioList = true; q.nRatios = n_ratios; q.ratioUp = ratio_up; q.ratioDown = ratio_down; q.ratioOf = ratio_of;
    q.banded = n_bands != 0; q.nBands = n_bands; q.edgeHz = edge_hz; q.bandGain = band_gain;
    q.nItems = n_items; q.termOffset = term_offset; q.file = file; q.start = start; q.gain = gain; q.irOf = ir_of;
    q.spanFirst = span_first; q.spanLen = span_len; q.fadeIn = fade_in; q.fadeOut = fade_out;
    q.nChannelsOut = n_channels_out; q.stream = stream;
    return stft_call(s, q, StftArgs{n_fft, frame_window, n_frames, hop, mode, n_filters, bank}, format, out);
}

int mrc_pac_store_reverb_ms(mrc_pac_store* s, double* ms) {
    MRC_TRY(store_alive(s, "mrc_pac_store_reverb_ms"));
    if (ms) { ms[0] = s->reverbMs[0]; ms[1] = s->reverbMs[1]; }
    return MRC_OK;
}

int mrc_pac_store_stft_window(mrc_pac_store* s, int rate_divisor, int mix, int n_ratios, const int32_t* ratio_up,
                              const int32_t* ratio_down, int zeros, double rolloff, int n_bands, const double* edge_hz,
                              const double* band_gain, int64_t n_items, const int64_t* term_offset, const int64_t* file,
                              const int64_t* start, const double* gain, const int32_t* ratio_of, const int32_t* ir_of, int n_fft,
                              const double* frame_window, int64_t n_frames, int64_t hop, int mode, int n_filters, const double* bank,
                              int n_channels_out, int format, void* out, void* stream) {
    WindowRequest q{kStft, WindowRequest::kStft};
    q.rateDivisor = rate_divisor; q.mix = mix; q.zeros = zeros; q.rolloff = rolloff;
    q.ratioList = true; q.nRatios = n_ratios; q.ratioUp = ratio_up; q.ratioDown = ratio_down; q.ratioOf = ratio_of;
    q.banded = n_bands != 0; q.nBands = n_bands; q.edgeHz = edge_hz; q.bandGain = band_gain;
    q.nItems = n_items; q.termOffset = term_offset; q.file = file; q.start = start; q.gain = gain; q.irOf = ir_of;
    q.nChannelsOut = n_channels_out; q.stream = stream;
    return stft_call(s, q, StftArgs{n_fft, frame_window, n_frames, hop, mode, n_filters, bank}, format, out);
}

int mrc_pac_store_decode_window_routed(mrc_pac_store* s, int rate_divisor, int mix, int n_ratios, const int32_t* ratio_up,
                                       const int32_t* ratio_down, int zeros, double rolloff, int n_bands, const double* edge_hz,
                                       const double* band_gain, int64_t n_items, const int64_t* term_offset, const int64_t* file,
                                       const int64_t* start, const int32_t* ratio_of, const double* route_gain,
                                       const int32_t* route_ir, int64_t window, int n_channels_out, int format, void* out,
                                       void* stream) {
    WindowRequest q{kWinRouted, WindowRequest::kRouted};
    q.rateDivisor = rate_divisor; q.mix = mix; q.zeros = zeros; q.rolloff = rolloff;
    q.ratioList = true; q.nRatios = n_ratios; q.ratioUp = ratio_up; q.ratioDown = ratio_down; q.ratioOf = ratio_of;
    q.banded = n_bands != 0; q.nBands = n_bands; q.edgeHz = edge_hz; q.bandGain = band_gain;
    q.nItems = n_items; q.termOffset = term_offset; q.file = file; q.start = start; q.gain = route_gain; q.irOf = route_ir;
    q.nChannelsOut = 1; q.routeChannels = n_channels_out; q.stream = stream;
    return window_call(s, q, window, format, out);
}

int mrc_pac_store_stft_window_routed(mrc_pac_store* s, int rate_divisor, int mix, int n_ratios, const int32_t* ratio_up,
                                     const int32_t* ratio_down, int zeros, double rolloff, int n_bands, const double* edge_hz,
                                     const double* band_gain, int64_t n_items, const int64_t* term_offset, const int64_t* file,
                                     const int64_t* start, const int32_t* ratio_of, const double* route_gain,
                                     const int32_t* route_ir, int n_fft, const double* frame_window, int64_t n_frames, int64_t hop,
                                     int mode, int n_filters, const double* bank, int n_channels_out, int format, void* out,
                                     void* stream) {
    WindowRequest q{kStftRouted, WindowRequest::kStftRouted};
    q.rateDivisor = rate_divisor; q.mix = mix; q.zeros = zeros; q.rolloff = rolloff;
    q.ratioList = true; q.nRatios = n_ratios; q.ratioUp = ratio_up; q.ratioDown = ratio_down; q.ratioOf = ratio_of;
    q.banded = n_bands != 0; q.nBands = n_bands; q.edgeHz = edge_hz; q.bandGain = band_gain;
    q.nItems = n_items; q.termOffset = term_offset; q.file = file; q.start = start; q.gain = route_gain; q.irOf = route_ir;
    q.nChannelsOut = 1; q.routeChannels = n_channels_out; q.stream = stream;
    return stft_call(s, q, StftArgs{n_fft, frame_window, n_frames, hop, mode, n_filters, bank}, format, out);
}

int mrc_pac_store_route_info(mrc_pac_store* s, int64_t* counts) {
    MRC_TRY(store_alive(s, "mrc_pac_store_route_info"));
    for (int i = 0; counts && i < 3; ++i) counts[i] = s->routeInfo[i];
    return MRC_OK;
}

int mrc_pac_store_decode_window(mrc_pac_store* s, int64_t n_items, const int64_t* file, const int64_t* start, int64_t window,
                                int n_channels_out, int format, void* out, void* stream) {
    WindowRequest q{kWin, WindowRequest::kItems};
    q.nItems = n_items; q.file = file; q.start = start; q.nChannelsOut = n_channels_out; q.stream = stream;
    return window_call(s, q, window, format, out);
}

int mrc_pac_store_decode_window_reduced(mrc_pac_store* s, int rate_divisor, int64_t n_items, const int64_t* file,
                                        const int64_t* start, int64_t window, int n_channels_out, int format, void* out,
                                        void* stream) {
    WindowRequest q{kWinReduced, WindowRequest::kItems};
    q.rateDivisor = rate_divisor;
    q.nItems = n_items; q.file = file; q.start = start; q.nChannelsOut = n_channels_out; q.stream = stream;
    return window_call(s, q, window, format, out);
}

int mrc_pac_store_decode_window_mix(mrc_pac_store* s, int rate_divisor, int mix, int64_t n_items, const int64_t* file,
                                    const int64_t* start, int64_t window, int format, void* out, void* stream) {
    WindowRequest q{kWinMix, WindowRequest::kItems};
    q.rateDivisor = rate_divisor; q.mix = mix; q.mixAllowed = kMixOfOne;
    q.nItems = n_items; q.file = file; q.start = start; q.nChannelsOut = 1; q.stream = stream;
    return window_call(s, q, window, format, out);
}

int mrc_pac_store_decode_window_resampled(mrc_pac_store* s, int rate_divisor, int mix, int up, int down, int zeros, double rolloff,
                                          int64_t n_items, const int64_t* file, const int64_t* start, int64_t window,
                                          int n_channels_out, int format, void* out, void* stream) {
    WindowRequest q{kWinResampled, WindowRequest::kItems};
    q.rateDivisor = rate_divisor; q.mix = mix;
    q.resampled = true; q.up = up; q.down = down; q.zeros = zeros; q.rolloff = rolloff;
    q.nItems = n_items; q.file = file; q.start = start; q.nChannelsOut = n_channels_out; q.stream = stream;
    return window_call(s, q, window, format, out);
}

int mrc_pac_store_decode_window_sum(mrc_pac_store* s, int rate_divisor, int mix, int up, int down, int zeros, double rolloff,
                                    int64_t n_items, const int64_t* term_offset, const int64_t* file, const int64_t* start,
                                    const double* gain, int64_t window, int n_channels_out, int format, void* out, void* stream) {
    WindowRequest q{kWinSum, WindowRequest::kRows};
    q.rateDivisor = rate_divisor; q.mix = mix; q.up = up; q.down = down; q.zeros = zeros; q.rolloff = rolloff;
    q.nItems = n_items; q.termOffset = term_offset; q.file = file; q.start = start; q.gain = gain;
    q.nChannelsOut = n_channels_out; q.stream = stream;
    return window_call(s, q, window, format, out);
}

int mrc_pac_store_decode_window_shaped(mrc_pac_store* s, int rate_divisor, int mix, int up, int down, int zeros, double rolloff,
                                       int n_bands, const double* edge_hz, const double* band_gain, int64_t n_items,
                                       const int64_t* term_offset, const int64_t* file, const int64_t* start, const double* gain,
                                       int64_t window, int n_channels_out, int format, void* out, void* stream) {
    WindowRequest q{kWinShaped, WindowRequest::kRows};
    q.rateDivisor = rate_divisor; q.mix = mix; q.up = up; q.down = down; q.zeros = zeros; q.rolloff = rolloff;
    q.banded = true; q.nBands = n_bands; q.edgeHz = edge_hz; q.bandGain = band_gain;
    q.nItems = n_items; q.termOffset = term_offset; q.file = file; q.start = start; q.gain = gain;
    q.nChannelsOut = n_channels_out; q.stream = stream;
    return window_call(s, q, window, format, out);
}

int mrc_pac_store_decode_window_speeds(mrc_pac_store* s, int rate_divisor, int mix, int n_ratios, const int32_t* ratio_up,
                                       const int32_t* ratio_down, int zeros, double rolloff, int n_bands, const double* edge_hz,
                                       const double* band_gain, int64_t n_items, const int64_t* term_offset, const int64_t* file,
                                       const int64_t* start, const double* gain, const int32_t* ratio_of, int64_t window,
                                       int n_channels_out, int format, void* out, void* stream) {
    WindowRequest q{kWinSpeeds, WindowRequest::kRows};
    q.rateDivisor = rate_divisor; q.mix = mix; q.zeros = zeros; q.rolloff = rolloff;
    q.ratioList = true; q.nRatios = n_ratios; q.ratioUp = ratio_up; q.ratioDown = ratio_down; q.ratioOf = ratio_of;
    q.banded = n_bands != 0; q.nBands = n_bands; q.edgeHz = edge_hz; q.bandGain = band_gain;
    q.nItems = n_items; q.termOffset = term_offset; q.file = file; q.start = start; q.gain = gain;
    q.nChannelsOut = n_channels_out; q.stream = stream;
    return window_call(s, q, window, format, out);
}

int mrc_pac_store_stft_ms(mrc_pac_store* s, double* ms) {
    MRC_TRY(store_alive(s, "mrc_pac_store_stft_ms"));
    if (ms) ms[0] = s->stftMs;
    return MRC_OK;
}

int mrc_pac_store_block_energy(mrc_pac_store* s, int rate_divisor, int mix, int64_t n_sel, const int64_t* file,
                               int64_t* entry_offset, int64_t entry_cap, int64_t* entry_block, double* energy, void* stream) {
    return block_energy(s, BlockEnergyRequest{rate_divisor, mix, n_sel, file, entry_offset, entry_cap, entry_block, energy, stream});
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
