// CPU harness for mrcaudiocodec_amd/csrc/mrc_pac_stage.hpp, the pure parts of the `.pac` readers' host glue: the staging
// layout builder against the hand formula, the chunk locator on three files (with and without a caller's offset in front),
// and the slots and plan entries of whole files against counts written out by hand.  Built with sanitizers where the
// compiler has them.  Exit 0 and nothing on stderr: every check held.
#include "mrc_pac_stage.hpp"

#include <cstdio>

namespace {

int failures = 0;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

// every sequence of `depth` field sizes from the six: offsets and total against sum of ((size + A - 1) & ~(A - 1))
void check_layout(size_t A) {
    const size_t sizes[6] = {0, 1, 255, 256, 257, 4097};
    const int depth = 4;
    int idx[depth] = {};
    for (int n = 0; n < 6 * 6 * 6 * 6; ++n) {
        for (int k = 0, v = n; k < depth; ++k, v /= 6) idx[k] = v % 6;
        mrc::StageLayout lay(A);
        size_t want = 0, got[depth];
        for (int k = 0; k < depth; ++k) {
            got[k] = lay.add(sizes[idx[k]]);
            CHECK(got[k] == want && got[k] % A == 0);
            want += (sizes[idx[k]] + A - 1) & ~(A - 1);
            CHECK(lay.total() == want);
        }
        for (int k = 0; k + 1 < depth; ++k)      // a field of no bytes shares its offset with the next one
            CHECK((got[k + 1] == got[k]) == (sizes[idx[k]] == 0));
    }
    mrc::StageLayout typed(A);
    CHECK(typed.add<long long>(3) == 0 && typed.add<int>(0) == typed.total() && typed.total() == ((24 + A - 1) & ~(A - 1)));
}

// three files at {0, 1000, 1000 + k} behind `front` bytes of the caller's: only the differences enter
void check_locator(int64_t front, int64_t k) {
    const int64_t file_offset[4] = {front, front + 1000, front + 1000 + k, front + 1000 + k + 700};
    const std::vector<int64_t> base = mrc::pac_file_bases(file_offset, 3);
    CHECK(base.size() == 3 && base[0] == 0 && base[1] == 1000 && base[2] == 1000 + k);
    const struct { int64_t off, file, byte; } want[] = {
        {0, 0, 0},                               // the first byte of file 0
        {999, 0, 999},
        {1000, 1, 0},
        {1000 + k - 4, 1, k - 4},                // the last chunk of file 1: a length field alone
        {1000 + k, 2, 0},
        {1000 + k + 512, 2, 512},                // a chunk in file 2
    };
    for (const auto& w : want) {
        const mrc::ChunkPlace p = mrc::pac_locate_chunk(base, w.off);
        CHECK(p.file == w.file && p.byte == w.byte);
    }
}

struct File { int nch, nBlocks; int shape; };

// whole files as pac_plan_groups counts them: all but the last block of a stereo file of more than one block are joint
mrc::PacGroupCounts count(const std::vector<File>& files) {
    mrc::PacGroupCounts c;
    c.nSlots[3] = 77;                            // (stale: clear_counts starts over)
    c.clear_counts();
    for (const File& f : files) {
        const int nJoint = f.nch == 2 && f.nBlocks > 1 ? f.nBlocks - 1 : 0;
        for (int i = 0; i < f.nBlocks; ++i) c.add_block(f.shape, i < nJoint, f.nch);
    }
    return c;
}
void check_counts() {
    const int s = 2;                             // shape (S,L): groups 4 (joint) and 5, categories 8, 9 (joint channels) and 10
    struct Want { int64_t joint, single, cat0, cat1, cat2, total, entries; int groups; };
    const struct { std::vector<File> files; Want w; } cases[] = {
        {{{2, 4, s}}, {3, 2, 3, 3, 2, 5, 8, 2}},     // stereo, 4 blocks: 3 joint slots, the last block's 2 chunks
        {{{2, 1, s}}, {0, 2, 0, 0, 2, 2, 2, 1}},     // stereo, 1 block: non-joint
        {{{1, 3, s}}, {0, 3, 0, 0, 3, 3, 3, 1}},     // mono, 3 blocks
        {{}, {0, 0, 0, 0, 0, 0, 0, 0}},              // no file
    };
    for (const auto& c : cases) {
        const mrc::PacGroupCounts g = count(c.files);
        for (int k = 0; k < mrc::kPacGroups; ++k) CHECK(g.nSlots[k] == (k == 2 * s ? c.w.joint : k == 2 * s + 1 ? c.w.single : 0));
        for (int k = 0; k < 2 * mrc::kPacGroups; ++k)
            CHECK(g.nCat[k] == (k == 4 * s ? c.w.cat0 : k == 4 * s + 1 ? c.w.cat1 : k == 4 * s + 2 ? c.w.cat2 : 0));
        CHECK(g.totalSlots == c.w.total && g.nEntries() == c.w.entries && g.groupsUsed() == c.w.groups);
    }
    // two shapes in one call: a stereo file of 4 (L,L) blocks and a mono file of 3 (S,S) blocks; a left / right window parses
    // ONE chunk of a stereo file's last block
    const mrc::PacGroupCounts two = count({{2, 4, 0}, {1, 3, 3}});
    CHECK(two.nSlots[0] == 3 && two.nSlots[1] == 2 && two.nSlots[7] == 3 && two.totalSlots == 8 && two.nEntries() == 11);
    mrc::PacGroupCounts one;
    one.add_block(0, false, 1);
    CHECK(one.nSlots[1] == 1 && one.nCat[2] == 1 && one.totalSlots == 1);
}

}  // namespace

int main() {
    check_layout(16);
    check_layout(256);
    for (int64_t front : {(int64_t)0, (int64_t)123457}) check_locator(front, 812);
    check_counts();
    return failures ? 1 : 0;
}
