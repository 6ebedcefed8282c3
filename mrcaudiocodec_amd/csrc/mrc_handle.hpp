// The handle behind the C ABI and the helpers every translation unit of the host glue shares (mrc_api.cpp: the per-block
// and pipelined entry points; mrc_api_chain.cpp, mrc_api_chain_measured.cpp: the chained stream encode; mrc_api_decode.cpp,
// mrc_api_nmr.cpp, mrc_api_store.cpp: the decode side).  Not part of the ABI.
// Who frees what: every device buffer, page-locked buffer, event and stream is a member of an owning type below and goes
// with the handle (mrc_destroy deletes it); nothing here is freed by name.
#pragma once
#include "mrc_internal.hpp"
#include "mrc_pac_stage.hpp"

#include <cmath>
#include <limits>
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

namespace mrc {

// ---- Owning types.  Every device resource of a handle is a member of one of these: move-only, freed by its destructor,
// so a struct that gains a buffer or an event needs no list that frees it.  mrc_handle's destructor drains the streams
// first.  None of them may be declared at namespace or static scope: its destructor would run after the HIP runtime
// has gone.

// A buffer that only grows: reserve() keeps what it has when that is enough, else frees it and allocates with headroom
// (the old contents are lost).  Mem: how to allocate, how to free, how much headroom.
template <class Mem>
struct GrowBuf {
    void* p = nullptr;
    size_t cap = 0;
    GrowBuf() = default;
    GrowBuf(GrowBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    GrowBuf& operator=(GrowBuf&& o) noexcept {           // o leaves with what this held and frees it
        std::swap(p, o.p);
        std::swap(cap, o.cap);
        return *this;
    }
    ~GrowBuf() { reset(); }
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        reset();
        const size_t want = Mem::headroom(bytes);
        hipError_t e = Mem::alloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    template <class T> T* as() { return (T*)p; }

  private:
    void reset() {
        if (p) typename Mem::Free{}(p);
        p = nullptr; cap = 0;
    }
};
struct HostFree { void operator()(void* p) const { (void)hipHostFree(p); } };
struct DevMem {
    using Free = DevFree;
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static size_t headroom(size_t bytes) { return bytes + bytes / 8 + 256; }
};
struct PinnedMem {
    using Free = HostFree;
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static size_t headroom(size_t bytes) { return bytes + bytes / 4 + 4096; }
};
using DevBuf = GrowBuf<DevMem>;
// page-locked host staging of the small-batch host entry points (one copy each way instead of one per array)
using PinnedBuf = GrowBuf<PinnedMem>;
// one page-locked object (or array) the device writes and the host reads
template <class T> using PinnedPtr = std::unique_ptr<T, HostFree>;
template <class P> hipError_t pinned_alloc(P* out, size_t bytes) {
    void* p = nullptr;
    const hipError_t e = PinnedMem::alloc(&p, bytes);
    if (e == hipSuccess) out->reset((typename P::pointer)p);
    return e;
}

// An event / a stream: created on first use (create() on one that exists does nothing), used as the raw handle
struct Event {
    struct Destroy { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
    std::unique_ptr<std::remove_pointer_t<hipEvent_t>, Destroy> e;
    hipError_t create(unsigned flags = hipEventDefault) {
        if (e) return hipSuccess;
        hipEvent_t raw = nullptr;
        const hipError_t rc = hipEventCreateWithFlags(&raw, flags);
        if (rc == hipSuccess) e.reset(raw);
        return rc;
    }
    operator hipEvent_t() const { return e.get(); }
    hipError_t ms_until(hipEvent_t later, double* ms) const {   // both have completed
        float f = 0.f;
        const hipError_t rc = hipEventElapsedTime(&f, e.get(), later);
        if (rc == hipSuccess) *ms = f;
        return rc;
    }
};
struct Stream {
    struct Destroy { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };
    std::unique_ptr<std::remove_pointer_t<hipStream_t>, Destroy> s;
    hipError_t create(unsigned flags = hipStreamDefault) {
        if (s) return hipSuccess;
        hipStream_t raw = nullptr;
        const hipError_t rc = hipStreamCreateWithFlags(&raw, flags);
        if (rc == hipSuccess) s.reset(raw);
        return rc;
    }
    operator hipStream_t() const { return s.get(); }
};
// The events of a timed call: create() before the first record, ev[i] to record, elapsed(i, j) once both have completed
template <int N>
struct EventSet {
    Event ev[N];
    hipError_t create() {
        for (Event& e : ev)
            if (hipError_t rc = e.create(); rc != hipSuccess) return rc;
        return hipSuccess;
    }
    hipEvent_t operator[](int i) const { return ev[i]; }
    hipError_t elapsed(int i, int j, double* ms) const { return ev[i].ms_until(ev[j], ms); }
};

static_assert(!std::is_copy_constructible_v<DevBuf> && std::is_nothrow_move_constructible_v<DevBuf>);
static_assert(!std::is_copy_constructible_v<PinnedBuf> && std::is_nothrow_move_constructible_v<PinnedBuf>);
static_assert(!std::is_copy_constructible_v<Event> && std::is_nothrow_move_constructible_v<Event>);
static_assert(!std::is_copy_constructible_v<Stream> && std::is_nothrow_move_constructible_v<Stream>);

// encode_host with few blocks (the per-block seam): one device layout, one page-locked copy each way (see encode_host)
struct SmallBatchBufs {
    DevBuf layout;                   // inputs, scan descriptor, reservoirs and results of the call, back to back
    DevBuf ev, pre;                  // chain_prep_kernel's grant events and the bits spent before each
    DevBuf table;                    // the scan's table ids (all 15: no pricing)
    DevBuf ctl;                      // mrc_dev_alloc_quant_chained: scan descriptor, items, item starts ...
    PinnedBuf ctlPin;                // ... their page-locked staging ...
    Event ctlCopied;                 // ... and the copy between the two, waited for before the staging is refilled
    PinnedBuf pinIn, pinOut;
};

// intermediate results of one encode call (lines, SMRs, band peaks); one set per stream that encodes concurrently
struct Workspace {
    DevBuf lines, smr, peak;
};

// The pipelined host entry point runs THREE streams -- one that only copies in, one that only launches kernels, one that
// only copies out -- over a ring of chunk buffers (lanes), ordered by events: measured on the MI355X box, page-locked
// copies reach 42-48 GB/s each way with ONE stream per direction and drop to 19-25 GB/s with three streams that each
// copy both ways (tools/pcie_rates.py), which is what one-stream-per-chunk pipelining amounts to.
struct Lane {
    DevBuf pcmL, pcmR, resIn, oScale, ms, ba, sf, mant, resOut;
    DevBuf pacBytes, pacOffs, pacTable, pacSaved;                // mrc_encode_stream_pcm16_pac: the chunk's packed form
    PinnedPtr<long long[]> pacTotal;                             // page-locked: the chunk's byte count, read by the host
    Event evIn, evK, evOut;                                      // chunk copied in / encoded / copied out (no timing)
};
constexpr int kLanes = 4;          // chunk buffers in flight (mrc_encode_stream_pcm16_pac reads sizes two chunks behind)
constexpr int kKernelEvents = 6;   // boundaries of: mdct | smr | band_stats | bitalloc | quantize

// Device state of one block-shape group of the chained encode (mrc_api_chain.cpp): the reservoir-free results (phase A),
// the sorted grant events of the bit allocation, and the outputs of the serial scan (phase B)
struct ChainGroupBufs {
    DevBuf offsets, lines, oscale, smr, peak, ms;                // phase A
    DevBuf ev, pre;                                              // prepared for phase B
    DevBuf bitAlloc, scaleFactor, mant, table, chunkMap;         // phase B outputs, packer inputs
};
struct ChainBufs {
    ChainGroupBufs g[kChainGroups];
    DevBuf pcmL, pcmR, flushPcm, items, itemStart, reservoir, groupDesc, packWs, out, hdr, chunkStream, resTrace, firstChunk,
        streamPos;
    EventSet<4> evT;                 // phase timing: start | phase A done | phase B done | packed
    int64_t lastTotal = -1;          // bytes the last mrc_encode_chained_stream_pac left in `out` (-1: none) -- mrc_chain_fetch_output
    const void* lastSrc = nullptr;   // ... or, after mrc_encode_chained_target_nmr_pac, in TargetBufs::sel (null: in `out`)
};

// Encode to a target noise-to-mask ratio (mrc_encode_chained_target_nmr_pac, mrc_api_chain_measured.cpp): reused from call to call
struct TargetBufs {
    DevBuf lines, thresh, oscale, smr;   // source analysis of one batch of blocks of one shape: X, T, overall scale, SMR (unused)
    DevBuf flushOffs;                // where Close()'s blocks start in ChainBufs::flushPcm
    DevBuf stat;                     // [rungs][chunks of the streams being decided][2]: max r_j, b * mean r_j
    DevBuf fileTab, fileOut, span;   // nmr_file_kernel's pseudo-files and sums; the gather's spans
    DevBuf keep;                     // a stream cut into time slabs: the packed bytes of all rungs until its last slab decides
    DevBuf sel;                      // the chosen files of the call, contiguous in stream order
    EventSet<6> ev;                  // NMR kernels of a slab | file reduction | gather, start and end each
    double ms[4] = {0, 0, 0, 0};     // phase A + preparation | scan | NMR (threshold pass included) | pack + gather
};

// Constant-quality VBR (mrc_encode_vbr_nmr_pac, mrc_api_chain_measured.cpp).  The source analysis and the file reduction use TargetBufs.
struct VbrBufs {
    DevBuf capped;                   // [chunks of the streams being decided]: capped bands, at a block's first chunk
    std::vector<Event> ev;           // start and end of every allocator (or profile) launch of a slab
    size_t evUsed = 0;
    double ms[4] = {0, 0, 0, 0};     // phase A + source analysis | the allocator | pack | all three
    // mrc_encode_vbr_size_pac: the slab's record per block-shape group, the streams' ceilings and file sizes of a probe
    DevBuf prof[kChainGroups], profPick[kChainGroups], ceilings, bytes;
    EventSet<3> evSize;              // the probes start | the final pick starts | it ended
    double sizeMs[5] = {0, 0, 0, 0, 0};   // phase A + source analysis | profile | probes | final pick + pack | their sum
    // mrc_dev_vbr_alloc / _profile / _pick: the identity chunk map and the chunks' streams, their page-locked staging and the
    // copy between the two (waited for before the staging is refilled)
    DevBuf stageMap;
    PinnedBuf stagePin;
    Event stageCopied;
};

// Device decode of whole `.pac` files (mrc_api_decode.cpp): reused from call to call
struct DecodeBufs {
    DevBuf consts;                   // UnpackTables + the band tables of the four block shapes (built once)
    UnpackBands bands{};             // ... with device pointers into consts
    DevBuf in;                       // one H2D copy: bytes | plan | group descriptors | block offsets | file tables
    DevBuf groups;                   // dense per-(shape, kind) arrays decode_kernel reads
    DevBuf x, pcm, err;              // decoded planes (float64), interleaved int16, UnpackErr (reset_unpack_err)
    PinnedBuf pinIn, pinOut;
    PinnedPtr<UnpackErr> pinErr;     // page-locked copy of err (read_unpack_err)
    EventSet<5> ev;                  // start | copied in | unpacked | synthesised | copied out
    double ms[4] = {0, 0, 0, 0};
};

// Noise-to-mask ratio of `.pac` files against their source (mrc_api_nmr.cpp): reused from call to call.  The parsing
// tables, the error word and its page-locked copy are DecodeBufs' (pac_parse).
struct NmrBufs {
    DevBuf in;                       // one H2D copy (NmrStage): bytes | plan | groups | entries | analyses | file table | sources
    DevBuf groups;                   // dense per-(shape, kind) arrays of the parsed chunks
    DevBuf planes;                   // padded int16 source planes
    DevBuf lines, thresh, oscale, smr;   // source analysis per shape: X, T, overall scale, SMR (unused)
    DevBuf out;                      // one D2H copy (NmrStage): per-file summaries | band noise | band mask
    DevBuf stat;                     // per entry: max r_j, b * mean r_j
    PinnedBuf pinIn, pinOut;
    EventSet<5> ev;                  // start | copied in | unpacked | source analysed | reduced and copied out
    double ms[4] = {0, 0, 0, 0};
};

// Windows of resident `.pac` files (mrc_pac_store_*, mrc_api_store.cpp): the workspace of one slab of each of its loops, reused
// from slab to slab and from call to call -- the loops nest (STFT over reverb over units), so each has buffers of its own.  The
// parsing tables, the error word and its page-locked copy are DecodeBufs' (pac_parse).
struct ResampleTable {               // the filter of one (up, down, zeros, rolloff), uploaded once (mrc_resample_taps.hpp)
    DevBuf taps;                     // [2 W][up]
    int W = 0, evenOdd = 0, skew = 0;   // half width; resample_out_kernel's LDS layout (resample_lds_layout)
    int skewNatural = 0;             // the better skew under the natural lane map (resample_multi_sum_out_kernel)
};
struct StoreNeed { int64_t item, file, block; };   // a block a slab must parse; item: index in the slab
struct StoreBufs {
    std::map<std::tuple<int, int, int, double>, ResampleTable> resample;   // mrc_pac_store_decode_window_resampled's filters
    // The host planner's scratch, cleared per slab and kept between slabs and calls: megabytes at thousands of items, which
    // a call would otherwise allocate and free each time -- and whether the C library then gives the pages back and faults
    // them in again at the next call depends on the history of the process, not on the call.
    std::vector<StoreNeed> needs;
    std::vector<WindowItem> items;
    std::vector<BandItem> bandItems;
    std::vector<int64_t> firstTile;
    std::vector<EnergyEntry> entries[kUnpackGroups];
    DevBuf in;                       // one H2D copy per slab (a StageLayout): plan | group descriptors | block offsets | items
                                     // (| the items' output starts: decode_window_resampled)
    DevBuf groups;                   // dense per-(shape, kind) arrays of the parsed chunks
    DevBuf planes;                   // float64, window + 4 n_mdct_lines samples per item and decoded channel
    PinnedBuf pinIn;                 // written again only after the slab that read it has been synchronised
    EventSet<6> ev;                  // start | plan uploaded | unpacked ; synthesis starts | planes done | windows written
    // the reverb loop (reverb_loop): a slab's dry terms [term][channel][window + pre-roll] (float64, written by the units
    // loop), the spectra of its convolved terms' segments, the term and source records (one H2D copy per slab from
    // their page-locked staging), the twiddle quadrant of the N-point transform (once per handle)
    DevBuf reverbDry, reverbSpec, reverbIn, reverbTw;
    PinnedBuf reverbPin;
    EventSet<3> reverbEv;            // forward transforms start | fold starts | windows written
    // the STFT loop (stft_loop): a slab's rows [row][channel][L] (float64, written by the reverb loop, whose own scratch is
    // in use underneath), and the call's tables in one allocation: twiddles | frame window | bank weights | bank supports
    DevBuf stftRows, stftTab;
    EventSet<2> stftEv;              // stft_kernel starts | ended
};

// ---- the host plan of whole `.pac` files, shared by mrc_decode_pac_pcm16 and mrc_pac_nmr (mrc_api_decode.cpp)
// Blocks are grouped exactly as pacfile.decode_pac groups them: a stereo file of more than one block is joint blocks
// followed by the two non-joint chunks Close() wrote, every other file is non-joint blocks.  A group is a (block shape,
// kind): group = shape * 2 + (non-joint), shapes in the order of UnpackBands: (L,L), (L,S), (S,L), (S,S).  The slots and plan
// entries a block takes are PacGroupCounts::add_block's (mrc_pac_stage.hpp).
static_assert(kPacGroups == kUnpackGroups);
struct PacFilePlan {
    int nch = 0;
    int64_t firstChunk = 0, nChunks = 0;   // into the call's chunk list
    int64_t xStart = 0, extent = 0, total = 0;   // where the file's decoded plane starts; its length; last start + a + b
};
struct PacPlan : PacGroupCounts {
    // pac_plan_scan
    std::vector<PacFilePlan> files;
    std::vector<int64_t> fileBase;         // [files]: where each file starts, relative to the first file's first byte
    std::vector<int64_t> chunkOff;         // relative to the first file's first byte
    std::vector<unsigned char> chunkShape;
    int64_t planeStride = 0;               // sum of the files' extents
    bool anyStereo = false;
    // pac_plan_groups: nSlots, nCat, totalSlots (PacGroupCounts), then pac_plan_layout
    int64_t slotBase[kUnpackGroups] = {};
    const HostShape* hs[4] = {};
    size_t gOff[kUnpackGroups][5] = {}, gBytes = 0;   // the groups' dense arrays in one device allocation
    int64_t nChunks() const { return (int64_t)chunkOff.size(); }
    int64_t nBlocks(int64_t f) const { return files[(size_t)f].nChunks / files[(size_t)f].nch; }
    int64_t nJoint(int64_t f) const {
        const PacFilePlan& fi = files[(size_t)f];
        return (fi.nch == 2 && fi.nChunks / 2 > 1) ? fi.nChunks / 2 - 1 : 0;
    }
    int shape(int64_t f, int64_t i) const {
        const PacFilePlan& fi = files[(size_t)f];
        return chunkShape[(size_t)(fi.firstChunk + i * fi.nch)];
    }
};

// block shapes in the order of UnpackBands: (L,L), (L,S), (S,L), (S,S)
inline void shape_ab(const mrc_config& c, int s, int* a, int* b) {
    *a = (s & 2) ? c.n_short : c.n_mdct_lines;
    *b = (s & 1) ? c.n_short : c.n_mdct_lines;
}
UnpackParams unpack_params(const mrc_config& c);
int ensure_decode_consts(mrc_handle* h);           // decode tables + the four shapes' band tables, once per handle
void decode_band_counts(const mrc_config& c, int nBands[4], std::vector<int>* cnt /* nullable: [4] */);   // host only
// The error word of a parse: err <- {0, INT_MAX} on the stream before the unpack kernel; behind it, the copy back and the
// wait: *bad = null when every chunk parsed, else the word (why, and the lowest bad chunk).  Shared by pac_parse and
// mrc_dev_unpack_blocks, which differ in how they name the chunk.
int reset_unpack_err(mrc_handle* h, hipStream_t st);
int read_unpack_err(mrc_handle* h, hipStream_t st, const UnpackErr** bad);
const char* unpack_status_text(int flag);
// the preamble of every call that takes a list of files: offsets that do not decrease, bytes where there are files
int check_file_list(mrc_handle* h, const char* fn, int64_t n_files, const uint8_t* buf, const int64_t* file_offset);
void copy_host(void* dst, const void* src, size_t n);   // memcpy over a few host threads for large copies
// headers, the handle's parameters, chunk scan with shape bits, block positions (host only: no device state is read or
// touched).  fn names the entry point in errors.
int pac_plan_scan(mrc_handle* h, const char* fn, int64_t n_files, const uint8_t* buf, const int64_t* file_offset,
                  PacPlan* p);
// ... one file of it, also behind mrc_pac_index (h == nullptr, hc the caller's cfg, owner = who named hc's values in the
// refusal of a file with other parameters): appends the file's chunks, their offsets counted from `base` bytes before the
// file, and fills *fi except xStart
int pac_scan_file(mrc_handle* h, const mrc_config& hc, const char* fn, const char* owner, int64_t f, const uint8_t* fb,
                  int64_t flen, int64_t base, std::vector<int64_t>* chunkOff, std::vector<unsigned char>* chunkShape,
                  PacFilePlan* fi);
// slots per group (pac_plan_groups: of whole files), then the shapes' tables and the layout of the groups' dense arrays
// (pac_plan_layout: from nSlots / nCat as they stand)
int pac_plan_groups(mrc_handle* h, const char* fn, PacPlan* p);
int pac_plan_layout(mrc_handle* h, const char* fn, PacPlan* p);
// the group descriptors, with gBase the device address of the dense arrays
inline void pac_plan_group_descs(const DecodeBufs& d, const PacPlan& p, UnpackGroupDev* gd, unsigned char* gBase) {
    for (int g = 0; g < kUnpackGroups; ++g) {
        const int s = g / 2;
        UnpackGroupDev& G = gd[g];
        G.shape = s;
        G.joint = !(g & 1);
        G.nb = d.bands.nBands[s] > 0 ? d.bands.nBands[s] : 0;
        G.halfN = d.bands.halfN[s];
        int** ptr[5] = {&G.oscale, &G.ms, &G.sf, &G.ba, &G.mant};
        for (int k = 0; k < 5; ++k) *ptr[k] = (int*)(gBase + p.gOff[g][k]);
    }
}
// Staging of the parse of whole files: the plan entries (ordered by (group, joint channel), so that a wave parses one kind)
// and the group descriptors.  visit(f, i, g, slot, ch, start) once per joint block (ch = 0; the slot holds both channels)
// and once per channel of a non-joint block; start = p_i, the block's position in its file.
template <class Visit>
void pac_plan_fill(const mrc_config& cfg, const DecodeBufs& d, const PacPlan& p, UnpackPlanEntry* plan, UnpackGroupDev* gd,
                   unsigned char* gBase, Visit visit) {
    int64_t catPos[2 * kUnpackGroups];
    for (int64_t k = 0, q = 0; k < 2 * kUnpackGroups; q += p.nCat[k], ++k) catPos[k] = q;
    pac_plan_group_descs(d, p, gd, gBase);
    int64_t slotNext[kUnpackGroups] = {};
    for (int64_t f = 0; f < (int64_t)p.files.size(); ++f) {
        const PacFilePlan& fi = p.files[(size_t)f];
        const int64_t nb = p.nBlocks(f), nJoint = p.nJoint(f);
        int64_t start = 0;
        for (int64_t i = 0; i < nb; ++i) {
            const int64_t c0 = fi.firstChunk + i * fi.nch;
            const int s = p.chunkShape[(size_t)c0];
            if (i < nJoint) {
                const int g = s * 2;
                const int slot = (int)slotNext[g]++;
                plan[catPos[s * 4]++] = UnpackPlanEntry{p.chunkOff[(size_t)c0], g * 2, slot};
                plan[catPos[s * 4 + 1]++] = UnpackPlanEntry{p.chunkOff[(size_t)c0 + 1], g * 2 + 1, slot};
                visit(f, i, g, slot, 0, start);
            } else {
                const int g = s * 2 + 1;
                for (int ch = 0; ch < fi.nch; ++ch) {
                    const int slot = (int)slotNext[g]++;
                    plan[catPos[s * 4 + 2]++] = UnpackPlanEntry{p.chunkOff[(size_t)c0 + ch], g * 2, slot};
                    visit(f, i, g, slot, ch, start);
                }
            }
            int a, b;
            shape_ab(cfg, s, &a, &b);
            start += a;
        }
    }
}

}  // namespace mrc

// A resident store (mrc_pac_store_create): the files' bytes on the handle's device, their index on the host.  It belongs to
// its handle, whose destructor takes the bytes back and clears `h`: what is left is a husk that refuses every call until
// mrc_pac_store_destroy deletes it.
struct mrc_pac_store {
    mrc_handle* h = nullptr;
    mrc::DevBuf bytes;               // the files back to back, as the caller passed them
    int64_t nBytes = 0;
    mrc::PacPlan index;              // pac_plan_scan's: files and where they start in `bytes`, chunk offsets into it, chunk shapes
    std::vector<int64_t> blockStart; // per block of every file, file after file: a_0 + .. + a_{i-1}
    std::vector<int64_t> firstBlock; // [files + 1] into blockStart
    std::vector<int64_t> tileEdge;   // file f with blocks: nBlocks(f) + 1 edges from firstBlock[f] + f on, in DOUBLED output samples:
                                     // block i's tile is [2 p_i + a_i - 2 L, 2 p_i + 2 a_i + b_i - 2 L), and tiles abut
    // mrc_pac_store_set_irs: the bank's partition spectra, response after response (N double2 per partition of B taps:
    // 32 bytes per tap, rounded up to whole partitions), and per response its length and first partition
    mrc::DevBuf irBank;
    std::vector<int64_t> irLen, irPart;
    // The statistics of the last call.  The store is the accumulator: a window entry zeroes what it reports, every slab of
    // every loop it runs adds to it, and the reverb and STFT kernels' times are counted into ms[3] once, at the end.
    double reverbMs[2] = {0, 0};     // last decode_window_reverb or stft_window: reverb_forward_kernel | reverb_fold_kernel
    double stftMs = 0;               // last stft_window: stft_kernel, summed over the slabs
    int64_t routeInfo[3] = {0, 0, 0};   // last routed call: forward segments transformed, inverse transforms, bytes of spectra
    int64_t stats[4] = {0, 0, 0, 0}; // last decode_window: chunks parsed, decode_kernel launches, slabs, plan bytes uploaded
    double ms[4] = {0, 0, 0, 0};     // ... plan upload | unpack | synthesis | window_out_kernel (resampled: resample_out_kernel)
                                     // (after block_energy: block_energy_kernel launches in [1]; ms: upload | unpack | that kernel | 0;
                                     // after band_energy_window: band_energy_kernel launches; upload | unpack | band sums | frames;
                                     // after filterbank_window: the same with filterbank_energy_kernel and the filter sums)
};

struct mrc_handle {
    mrc_config cfg{};
    int device = 0;
    mrc::Stream stream;
    std::map<std::pair<int, int>, mrc::HostShape> shapes;
    std::map<std::tuple<int, int, int>, mrc::HostShape> synthShapes;   // (a, b, D): synthesis-only shape (a / D, b / D), get_synth_shape
    std::string error;
    mrc::Workspace ws;               // workspace of mrc_dev_encode* (calls on one handle are serialised)
    mrc::Lane lanes[mrc::kLanes];    // mrc_encode_stream_pcm16: chunk buffers ...
    mrc::Stream stIn, stOut;         // ... and its copy-in / copy-out streams; the kernels of all chunks run
    mrc::Workspace wsPipe;           //     on `stream`, one after the other: one workspace.  (No third stream of its own:
                                     //     the runtime multiplexes streams onto 4 hardware queues by default -- with the
                                     //     null stream and `stream` that is exactly four; a fifth would share a queue with
                                     //     one of the others and serialise with it: 10 000 instead of 19 000 Msamples/s)
    std::vector<mrc::DevBuf> stage;  // staging of the host entry points: handed out in order by a Stage (mrc_api.cpp)
    mrc::SmallBatchBufs smallBatch;  // ... except encode_host with few blocks
    mrc::DevBuf sos;                 // mrc_dev_transient_peaks: the filter coefficients
    mrc::DevBuf packWs;              // mrc_dev_pack_blocks: chunk sizes / positions / (table ids)
    int64_t packLastChunks = 0, packLastCap = 0;   // ... of the most recent call (mrc_dev_pack_status)
    mrc::ChainBufs chain;            // mrc_encode_chained_*: see mrc_api_chain.cpp
    mrc::DecodeBufs dec;             // mrc_dev_unpack_blocks / mrc_decode_pac_pcm16: see mrc_api_decode.cpp
    mrc::NmrBufs nmr;                // mrc_pac_nmr: see mrc_api_nmr.cpp
    mrc::TargetBufs target;          // mrc_encode_chained_target_nmr_pac: see mrc_api_chain_measured.cpp
    mrc::VbrBufs vbr;                // mrc_encode_vbr_nmr_pac: see mrc_api_chain_measured.cpp
    mrc::StoreBufs store;            // mrc_pac_store_decode_window: see mrc_api_store.cpp
    std::vector<mrc_pac_store*> stores;   // the live stores of this handle (not owned: mrc_pac_store_destroy deletes them)
    int64_t storeSlabSamples = (int64_t)1 << 24;   // mrc_set_option(MRC_OPT_STORE_SLAB_SAMPLES)
    int storeRouteGroup = 0;         // mrc_set_option(MRC_OPT_STORE_ROUTE_GROUP): channels per workgroup of reverb_route_fold_kernel; 0: per slab
    double chainMs[4] = {0, 0, 0, 0};   // last chained encode: phase A, phase B, pack, whole call (host clock)
    bool timing = false;
    bool exactSpread = false;        // mrc_set_option(MRC_OPT_EXACT_SPREAD)
    bool smrAllBands = false;        // mrc_set_option(MRC_OPT_SMR_ALL_BANDS)
    int chainThreads = 0;            // mrc_set_option(MRC_OPT_CHAIN_THREADS): workgroup size of the serial scan, 0 = by stream count
    int64_t chainSlabBlocks = 131072; // mrc_set_option(MRC_OPT_CHAIN_SLAB_BLOCKS): blocks per slab of a chained encode (~7.5 GB of device memory)
    bool chainForceFallback = false; // mrc_set_option(MRC_OPT_CHAIN_FORCE_REPAIR): tests of chain_prep_kernel's repair pass
    bool sensOn = false;             // mrc_set_option(MRC_OPT_SENSITIVITY): count decisions near a rounding edge ...
    mrc::DevBuf sens;                // ... here: MRC_SENS_COUNT counters (uint64), mrc_get_sensitivity
    int sensMode = 0;                // the option's value as set (0, 1 or 2), what mrc_get_option returns
    mrc::EventSet<mrc::kKernelEvents> ev;   // per-kernel timing: see collect_kernel_ms (mrc_api.cpp)
    double stageMs[3] = {0, 0, 0};
    double kernelMs[5] = {0, 0, 0, 0, 0};
    // The members free themselves, on the handle's device and once nothing queued can still touch them: that is said
    // here, not left to the order of the declarations above.
    ~mrc_handle() {
        (void)hipSetDevice(device);
        for (hipStream_t st : {(hipStream_t)stream, (hipStream_t)stIn, (hipStream_t)stOut})
            if (st) (void)hipStreamSynchronize(st);
        for (mrc_pac_store* s : stores) {
            s->bytes = mrc::DevBuf();
            s->irBank = mrc::DevBuf();
            s->h = nullptr;
        }
    }
};

namespace mrc {

// error text of the last failed mrc_create (no handle exists yet)
std::string& create_error();

inline int fail(mrc_handle* h, int code, const std::string& msg) {
    if (h) h->error = msg; else create_error() = msg;
    return code;
}
inline int hip_fail(mrc_handle* h, hipError_t e, const char* what) {
    return fail(h, MRC_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define MRC_HIP(h, call)                                              \
    do {                                                              \
        hipError_t e_ = (call);                                       \
        if (e_ != hipSuccess) return mrc::hip_fail((h), e_, #call);   \
    } while (0)
#define MRC_TRY(expr)              \
    do {                           \
        int rc_ = (expr);          \
        if (rc_ != MRC_OK) return rc_; \
    } while (0)

// THE parse step of the `.pac` readers: event, the staging copy to the device, event, unpack_dense_kernel over the plan,
// event, the verdict.  The caller says where its staging lives and where the plan entries and group descriptors sit in
// it, and which device bytes the entries point into: the staging itself (whole-file decode, NMR) or a store's resident
// bytes.  A bad chunk is refused as "<fn>: file F: chunk at byte B: <reason>", F and B from pac_locate_chunk over
// fileBase (PacPlan::fileBase of the files the offsets count in).
struct PacParse {
    const void* pin;                 // the staging: page-locked host copy, device copy, bytes
    void* dev;
    size_t total, oPlan, oGroups;    // ... and where its plan entries [nChunks] and group descriptors [kUnpackGroups] sit
    int64_t nChunks;
    const uint8_t* bytes;            // device: what the entries' offsets point into, and its length
    int64_t nBytes;
    hipEvent_t ev[3];                // recorded: before the copy | copied | unpacked
    hipStream_t st;
};
int pac_parse(mrc_handle* h, const char* fn, const std::vector<int64_t>& fileBase, const PacParse& p);

// Every group of the plan that has slots: launch(g, its descriptor, its slots' offsets on the device).  gd: the host copy
// of the descriptors, offs: the device offsets of all slots, group after group (slotBase).
template <class Launch>
int pac_for_groups(mrc_handle* h, const PacPlan& pl, const UnpackGroupDev* gd, const int64_t* offs, Launch launch) {
    for (int g = 0; g < kUnpackGroups; ++g)
        if (pl.nSlots[g]) MRC_HIP(h, launch(g, gd[g], offs + pl.slotBase[g]));
    return MRC_OK;
}
// ... decode_kernel for each (full rate, a plane per channel): channel 0 into x, channel 1 of a joint slot planeStride behind
inline int decode_groups(mrc_handle* h, const PacPlan& pl, const UnpackGroupDev* gd, const int64_t* offs, double* x,
                         int64_t planeStride, hipStream_t st) {
    return pac_for_groups(h, pl, gd, offs, [&](int g, const UnpackGroupDev& G, const int64_t* o) {
        return launch_decode(pl.hs[g / 2]->dev, pl.nSlots[g], G.joint ? 2 : 1, G.oscale, G.joint ? G.ms : nullptr, G.sf, G.ba,
                             G.mant, o, x, G.joint ? x + planeStride : nullptr, st);
    });
}

// Whichever way a function is left, nothing it queued on these streams still touches the caller's memory or the host
// temporaries declared before the guard.  (Null entries are skipped.)
struct DrainGuard {
    hipStream_t st[3];
    ~DrainGuard() { for (hipStream_t s : st) if (s) (void)hipStreamSynchronize(s); }
};

// every entry point that launches comes through here first: the launches, the tables and the caller's pointers all
// belong to the handle's device, whatever the calling thread's current device was
int get_shape(mrc_handle* h, int a, int b, const HostShape** out);
// the synthesis-only shape (a / D, b / D) of the reduced-rate store decode (build_synth_shape), cached per (a, b, D);
// synth_shape_refusal: why there is none, D and the shape named -- empty if there is one (host only)
std::string synth_shape_refusal(int a, int b, int D);
int get_synth_shape(mrc_handle* h, int a, int b, int D, const HostShape** out);
inline bool all_bands_non_empty(const HostShape& hs) {
    for (int n : hs.bandN) if (n <= 0) return false;
    return true;
}
inline hipStream_t pick_stream(mrc_handle* h, void* stream) { return stream ? (hipStream_t)stream : h->stream; }

// the device packer's settings for blocks of shape (a, b)
inline PackParams pack_params(const mrc_config& cfg, int a, int b, int nch, int joint, int use_huffman) {
    PackParams P;
    P.nch = nch; P.joint = joint ? 1 : 0; P.useHuffman = use_huffman ? 1 : 0;
    P.nScaleBits = cfg.n_scale_bits; P.nMantSizeBits = cfg.n_mant_size_bits;
    P.blkBitsA = cfg.blksw_bits_a; P.blkBitsB = cfg.blksw_bits_b;
    P.bitA = (unsigned)(1 - a / cfg.n_mdct_lines); P.bitB = (unsigned)(1 - b / cfg.n_mdct_lines);   // py2 int division
    return P;
}
inline const PackTables& host_pack_tables() {
    static const PackTables tables = [] { PackTables t; pack_tables(&t); return t; }();
    return tables;
}

// The chained back end (chain_prep_kernel + chain_phase_b_kernel), defined in mrc_api_chain.cpp.  Its scan covers <= 64
// coded bands, 2..16 mantissa bits and lines in units of four, at most kChainMaxLinesPerItem of them per block:
// chain_shape_misfit returns null when blocks of S with `nstream` channels fit, else which limit they break.
const char* chain_shape_misfit(const DevShape& S, int nstream);
// the scan's view of one block-shape group (joint: two channels with an M/S switch, else one channel)
ChainGroupDev chain_group_desc(const HostShape& hs, int joint, const double* lines, const double* peak, const int* oscale,
                               const int* ms, const unsigned* ev, const unsigned* pre, int* bitAlloc, int* scaleFactor,
                               unsigned short* mant, int* table);
// The scan's control data for n blocks of ONE group, cut into streams of blocksPerStream consecutive blocks (n a multiple of
// it): the descriptor, item i = block i of group 0, stream s = items [s blocksPerStream, (s + 1) blocksPerStream).  Host
// memory: desc [1], items [n], itemStart [n / blocksPerStream + 1].
void chain_one_group(const ChainGroupDev& D, int64_t n, int64_t blocksPerStream, ChainGroupDev* desc, int32_t* items,
                     long long* itemStart);

// phase A of the per-block path (windowed MDCT + overall scale -> [M/S switch] -> SMRs and per-band peaks), defined in
// mrc_api.cpp beside encode_core, which it is the first half of.  smr == nullptr: it stops behind the M/S switch.
int encode_phase_a(mrc_handle* h, const DevShape& S, int64_t n, const void* chL, const void* chR, int fmt, int64_t stride,
                   const int64_t* offsets, double* lines, int32_t* oscale, int32_t* msSwitch, double* smr, double* peak,
                   hipStream_t st, bool timing);

// ---- the noise-to-mask ratio's two ends, shared by mrc_pac_nmr (mrc_api_nmr.cpp) and the chained calls that measure their
// own output (mrc_api_chain_measured.cpp): the numbers of the latter are the former's to the bit because both come from here.
// The source analysis: n one-channel blocks of shape S at explicit offsets `offs` into the int16 samples `src` -> lines X
// [n][halfN], overall scales os [n], masked thresholds T [n][halfN] (the generic mode of smr_kernel that writes them;
// MRC_OPT_EXACT_SPREAD honoured), SMRs to smr [n][kMaxBands] (unused).
inline hipError_t launch_nmr_source(mrc_handle* h, const DevShape& S, int64_t n, const void* src, const int64_t* offs, double* X,
                                    int* os, double* smr, double* T, hipStream_t st) {
    const hipError_t e = launch_mdct(S, n, src, nullptr, kSampleI16, 0, offs, true, X, os, st);
    if (e != hipSuccess) return e;
    return launch_smr(S, n, src, nullptr, kSampleI16, 0, offs, X, os, smr, T, nullptr, nullptr, h->exactSpread, st);
}
// The file's values from nmr_file_kernel's row f = (max r, sum of b * mean r, disturbed blocks, -) and the file's weight
// (the sum of b over its blocks and channels): -inf where nothing was disturbed at all
struct NmrFileValues { double nmr_total_db, nmr_max_db; int64_t disturbed_blocks; };
inline NmrFileValues nmr_file_values(const double* f, int64_t weight) {
    const auto db = [](double v) { return v > 0.0 ? 10.0 * std::log10(v) : -std::numeric_limits<double>::infinity(); };
    return {db(weight > 0 ? f[1] / (double)weight : 0.0), db(f[0]), (int64_t)f[2]};
}

}  // namespace mrc
