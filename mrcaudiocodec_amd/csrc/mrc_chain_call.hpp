// What the two translation units of the chained encode share: mrc_api_chain.cpp (the chained core: schedule, one slab, the
// slab loop, the budgeted entry points) and mrc_api_chain_measured.cpp (the calls that measure their own output while a
// slab's planes are still on the device).  Not part of the ABI.
#pragma once
#include "mrc_handle.hpp"

#include <functional>
#include <string>
#include <vector>

namespace mrc {

struct ChainMeasure;

// One slab of a call (plan_slabs): streams s0 .. s0 + ns - 1 whole, or blocks [i0, i1) of the one stream s0 (a TIME slab);
// first / last: the stream's first / last slab
struct Slab { int64_t s0, ns; int64_t i0, i1; bool first, last, timeSlab; };

// One chained encode as its entry point received it, in the order of include/mrc_hip.h.  n_rates bit rates (rates == nullptr:
// one, the handle's target_bits_per_sample): phase A and the event lists once, the scan and the packer per (rate, stream).
// pcm_right == nullptr: mono streams.  Every per-stream / per-item array holds n_rates rows: reservoir_in / reservoir_out
// [R][n_streams], stream_byte_offset [R][n_streams + 1], item_byte_offset [R][n_items + 1], reservoir_trace [R][n_items],
// total_bytes [R]; byte offsets are relative to the start of their rate's output.  Where the bytes go is the layers' own.
struct ChainCall {
    int n_rates; const double* rates;
    int64_t n_streams;
    const void *pcm_left, *pcm_right; int sample_format; int64_t stream_stride;
    const int64_t *block_start, *block_offset; const int32_t *block_a, *block_b;
    const int32_t* reservoir_in; int use_huffman, with_flush; const uint32_t* num_samples;
    int64_t *stream_byte_offset, *item_byte_offset; int32_t *reservoir_out, *reservoir_trace; int64_t* total_bytes;
    void* stream;
    ChainMeasure* measure = nullptr; // a call that measures its own output: what its slabs do beside encoding
    int64_t slabBlocks = 0;          // the slab capacity of this call where it is not slab_cap's (mrc_encode_vbr_size_pac)
    const Slab* slab = nullptr;      // in a slab's call (chained_slabs sets it): the slab of the caller's call that it is
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

// What a call that measures its own output adds to its slabs (ChainCall::measure), as chained_core asks for it: a slab's
// call `c` (c.slab: which slab), its schedule, the blocks of every group, the stream everything is queued on.  The state
// every such call keeps from slab to slab is here too.
struct ChainMeasure {
    const int64_t* blockStart = nullptr;   // the caller's block_start (a slab's call has its own)
    int64_t unitChunks = 0;          // chunks of one rung of the streams being decided: the stride of TargetBufs::stat's rows
    std::vector<int64_t> flushOffs;  // Close()'s blocks in flushPcm (a queued copy reads it)
    double msMeasure = 0;            // device time of the measuring kernels, summed over the slabs
    // true: the call allocates itself where the serial scan would run (in_place_of_scan) -- phase A stops at the M/S switch:
    // no SMRs, no band peaks, no event lists, and the packer chooses the Huffman tables
    virtual bool allocates() const { return false; }
    virtual int in_place_of_scan(mrc_handle*, const ChainCall&, const ChainSchedule&, const int64_t*, hipStream_t) { return MRC_OK; }
    // queued behind the pack and the headers, while the scan's planes are in device memory
    virtual int behind_pack(mrc_handle*, const ChainCall&, const ChainSchedule&, const int64_t*, hipStream_t) { return MRC_OK; }
    // after the slab's synchronise: what is read from the events
    virtual int read_events(mrc_handle*) { return MRC_OK; }
    virtual ~ChainMeasure() = default;
};

int64_t vbr_size_slab_blocks(mrc_handle* h, int nch);            // blocks per slab of mrc_encode_vbr_size_pac (ChainCall::slabBlocks)

// The one argument check of a chained call: all that can be refused without reading the schedule (out, out_cap: an entry
// per rate).  A call that passes serves no earlier call's output any more (forget_held_output), whatever becomes of it.
int check_call(mrc_handle* h, const char* who, const ChainCall& c, uint8_t* const* out, const int64_t* out_cap);
void forget_held_output(mrc_handle* h);                           // mrc_chain_fetch_output has nothing to fetch
// the rates of a ladder, shared by every call that takes some: their number, then entry r (ascending: above entry r - 1)
int rate_count_check(mrc_handle* h, const std::string& w, int n_rates);
int rate_check(mrc_handle* h, const std::string& w, const double* rates, int r, bool ascending);
// stage the host PCM of a host-memory entry point in the handle's device buffers
int stage_pcm(mrc_handle* h, const ChainCall& c);

// A chained encode cut into slabs.  out_cap[r] is the room of rate r's output.  direct_out (one rate): a device buffer of
// out_cap[0] bytes the slabs write into in place; null: every slab packs into the handle's buffer and
// sink(the slab, rate r, its bytes are at `buf` on the device, n of them, they belong at byte `at` of rate r's output) -> status;
// after(the slab, its stream_byte_offset [R][ns + 1], where each rate's bytes start in `buf`, buf) -> status, once per slab
// behind its sinks.  An empty function: nothing to do.
using ChainSink = std::function<int(const Slab& sl, int r, uint8_t* buf, int64_t n, int64_t at)>;
using ChainAfter = std::function<int(const Slab& sl, const int64_t* sOff, const int64_t* base, const uint8_t* buf)>;
int chained_slabs(mrc_handle* h, const ChainCall& c, const int64_t* out_cap, uint8_t* direct_out, const ChainSink& sink,
                  const ChainAfter& after);
// The host-memory entry points: check_call, the PCM staged, every slab's bytes of rate r copied behind the previous slab's
// in out[r]
int chained_host(mrc_handle* h, const char* who, ChainCall c, uint8_t* const* out, const int64_t* out_cap,
                 const ChainAfter& after = {});

}  // namespace mrc
