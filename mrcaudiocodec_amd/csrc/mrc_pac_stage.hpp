// The pure parts of the `.pac` readers' host glue (mrc_api_decode.cpp, mrc_api_nmr.cpp, mrc_api_store.cpp): how a staging
// buffer is laid out, which file a chunk lies in, and how many slots and plan entries a block takes.  No HIP, no handle:
// tests/pac_stage_check.cpp compiles this header alone for the host.  What needs the handle is in mrc_handle.hpp.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

namespace mrc {

// The layout of one staging buffer: fields back to back, each at the next multiple of `align` (a power of two: 256 for
// what the readers upload, 16 for encode_host's small batch).  add() returns the field's offset; a field of no bytes takes
// no space and shares its offset with the next one.
struct StageLayout {
    size_t align, size = 0;
    explicit StageLayout(size_t a) : align(a) {}
    size_t add(size_t bytes) {
        const size_t at = size;
        size += (bytes + align - 1) & ~(align - 1);
        return at;
    }
    template <class T> size_t add(size_t count) { return add(sizeof(T) * count); }
    size_t total() const { return size; }
};

// Where the files of a call start, counted from the first file's first byte ([n_files] of the caller's [n_files + 1]
// offsets).  Chunk offsets of a plan count from the same byte.
inline std::vector<int64_t> pac_file_bases(const int64_t* file_offset, int64_t n_files) {
    std::vector<int64_t> base((size_t)n_files);
    for (int64_t f = 0; f < n_files; ++f) base[(size_t)f] = file_offset[f] - file_offset[0];
    return base;
}
// The file of the chunk at plan offset `off`: the last file whose base is at or before it; `byte` counts from that file's
// first byte.  (No file has a chunk before it starts; an empty list answers file 0.)
struct ChunkPlace { int64_t file, byte; };
inline ChunkPlace pac_locate_chunk(const std::vector<int64_t>& fileBase, int64_t off) {
    const int64_t f = std::max<int64_t>(0, std::upper_bound(fileBase.begin(), fileBase.end(), off) - fileBase.begin() - 1);
    return {f, fileBase.empty() ? off : off - fileBase[(size_t)f]};
}

// Slots and plan entries per (block shape, kind) group.  A group is group = shape * 2 + (non-joint), shapes in the order of
// UnpackBands: (L,L), (L,S), (S,L), (S,S).  A plan-entry category is shape * 4 + {joint channel 0, joint channel 1,
// non-joint, unused}: the plan is ordered by category so that a wave parses one kind.
constexpr int kPacGroups = 8;
struct PacGroupCounts {
    int64_t nSlots[kPacGroups] = {}, nCat[2 * kPacGroups] = {}, totalSlots = 0;
    void clear_counts() { *this = PacGroupCounts{}; }
    // THE block-kind rule: a joint block is one slot of two streams and one plan entry in each of two categories; any other
    // block is one slot and one plan entry per chunk parsed (all of its channels, or the one a caller asks for)
    void add_block(int shape, bool joint, int chunksParsed) {
        if (joint) { nSlots[shape * 2] += 1; nCat[shape * 4] += 1; nCat[shape * 4 + 1] += 1; }
        else { nSlots[shape * 2 + 1] += chunksParsed; nCat[shape * 4 + 2] += chunksParsed; }
        totalSlots += joint ? 1 : chunksParsed;
    }
    int64_t nEntries() const { return std::accumulate(nCat, nCat + 2 * kPacGroups, (int64_t)0); }   // = chunks parsed
    int groupsUsed() const { return kPacGroups - (int)std::count(nSlots, nSlots + kPacGroups, 0); }
};

}  // namespace mrc
