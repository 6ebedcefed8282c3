// CPU harness for mrcaudiocodec_amd/csrc/mrc_unpack.hpp (the chunk parser the device unpack kernel runs): parses the
// cases of an input file with unpack_fixed_chunk in the layout of mrc_unpack_blocks, so that the test can compare every
// integer and every accept / reject decision with the host parser.  Built with sanitizers where the compiler has them:
// each case's bytes sit in an allocation of exactly their length.
//
// input (little-endian):  uint16 lut[4 * 512], int32 escape[4], int32 nCases, then per case
//   int32 params[6] (nScaleBits, nMantSizeBits, blkBitsA, blkBitsB, nShort, nLines), int32 nBands[4], int32 halfN[4],
//   int32 bandN[nBands[s]] for s with nBands[s] > 0, int32 nBlocks, nch, joint, int64 len, uint8 bytes[len],
//   int64 chunkOffset[nBlocks * nch]
// output: per case int32 status (0 = accepted, else the first failing chunk's UnpackStatus), and if accepted
//   a[n], b[n], table[n][nch], oscale[n][joint ? 4 : nch], ms[n][32], sf[n][nch][32], ba[n][nch][32], mant[n][nch][nLines]
#include "mrc_unpack.hpp"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

namespace {

FILE* in;
FILE* out;

template <class T> void rd(T* p, size_t n) {
    if (n && std::fread(p, sizeof(T), n, in) != n) { std::fprintf(stderr, "short input\n"); std::exit(2); }
}
template <class T> T rd1() { T v; rd(&v, 1); return v; }
void wr(const int32_t* p, size_t n) { if (n) std::fwrite(p, sizeof(int32_t), n, out); }

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: unpack_check in out\n"); return 2; }
    in = std::fopen(argv[1], "rb");
    out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    mrc::UnpackTables T;
    rd(T.lut, mrc::kUnpackLutEntries);
    rd(T.escape, 4);
    const int nCases = rd1<int32_t>();
    for (int k = 0; k < nCases; ++k) {
        int32_t prm[6];
        rd(prm, 6);
        mrc::UnpackParams P{prm[0], prm[1], prm[2], prm[3], prm[4], prm[5]};
        mrc::UnpackBands B;
        rd(B.nBands, 4);
        rd(B.halfN, 4);
        std::vector<int> bandN[4];
        for (int s = 0; s < 4; ++s) {
            bandN[s].resize(B.nBands[s] > 0 ? B.nBands[s] : 0);
            rd(bandN[s].data(), bandN[s].size());
            B.bandN[s] = bandN[s].data();
        }
        const int64_t n = rd1<int32_t>();
        const int nch = rd1<int32_t>(), joint = rd1<int32_t>();
        const int64_t len = rd1<int64_t>();
        std::unique_ptr<uint8_t[]> buf(new uint8_t[len > 0 ? len : 1]);
        rd(buf.get(), (size_t)len);
        std::unique_ptr<int64_t[]> offs(new int64_t[n * nch + 1]);
        rd(offs.get(), (size_t)(n * nch));
        const int L = P.nLines, nOs = joint ? 4 : nch, MB = mrc::kUnpackMaxBands;
        std::vector<int32_t> a(n), b(n), table(n * nch), osc(n * nOs), ms(n * MB), sf(n * nch * MB), ba(n * nch * MB),
            mant(n * nch * L);
        mrc::UnpackFixedOut O{a.data(), b.data(), table.data(), osc.data(), ms.data(), sf.data(), ba.data(), mant.data()};
        int status = 0;
        for (int64_t blk = 0; blk < n && !status; ++blk)
            for (int ch = 0; ch < nch && !status; ++ch)
                status = mrc::unpack_fixed_chunk(buf.get(), len, offs.get(), blk, ch, nch, joint, P, B, T.lut, T.escape, O);
        wr(&status, 1);
        if (!status) {
            wr(a.data(), a.size()); wr(b.data(), b.size()); wr(table.data(), table.size()); wr(osc.data(), osc.size());
            wr(ms.data(), ms.size()); wr(sf.data(), sf.size()); wr(ba.data(), ba.size()); wr(mant.data(), mant.size());
        }
    }
    std::fclose(out);
    return 0;
}
