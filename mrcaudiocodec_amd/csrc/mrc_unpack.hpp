// The `.pac` channel-chunk parser as portable code: the device unpack kernel (mrc_kernels_unpack.hip) runs it one lane
// per chunk, and tests/unpack_check.cpp compiles the same source for the host (with sanitizers) to hold it against the
// host parser of mrc_pack.cpp (mrc_unpack_blocks + read_band_records), which stays the yardstick.
//
// Semantics of pacfileThem.py:176-302 (ReadDataBlock) and 341-560 (JointReadDataBlock) as mrc_unpack_blocks has them:
//   payload = table id : 4, block-switch bits : blksw_bits_a + blksw_bits_b, then
//     non-joint  overall scale : nScaleBits
//     joint ch0  overall scales L, R, M, S : 4 x nScaleBits, M/S switch : 1 bit per band
//   then per band {ba-1 | 0 : nMantSizeBits, scale factor : nScaleBits, mantissas: ba raw bits each, or Huffman codes
//   with the raw ba bits after the escape code}.  Bits are MSB first; a peek reads bytes past the payload as zero, a
//   read past its end is an error.  Also errors: a table id outside {0..3, 15}, a stored allocation above 16 bits,
//   peeked bits that are no code of the table, a block shape without a band table.
//
// Memory safety by construction: the reader loads byte i of the payload only for 0 <= i < nBytes; every write goes
// through the caller's pointers at indices below the shape's band count / line count and the caller's padding.
#pragma once
#include <cstdint>

#ifndef MRC_HD
#if defined(__HIPCC__)
#define MRC_HD __host__ __device__ __forceinline__
#else
#define MRC_HD inline
#endif
#endif

namespace mrc {

constexpr int kUnpackPeekBits = 9;                          // longest Huffman code of the four tables
constexpr int kUnpackLutEntries = 4 << kUnpackPeekBits;     // [table][next 9 bits] -> value | length << 8 (0: no code)
constexpr int kUnpackRawTable = 15;                         // codecThem.py:149
constexpr int kUnpackMaxBands = 32;                         // MRC_MAX_BANDS

enum UnpackStatus : int {
    kUnpackOk = 0,
    kUnpackTruncated = 1,       // a read past the payload, or a chunk that does not fit the buffer
    kUnpackBadTable = 2,        // table id 4..14
    kUnpackBadAlloc = 3,        // stored bit allocation > 16
    kUnpackBadCode = 4,         // no code of the table starts with the next bits
    kUnpackBadShape = 5,        // shape without a band table, or not the shape the caller expects / the block's other chunk has
};

// Decode tables: derived from mrc_huffman_tables.hpp by mrc_pack.cpp (mrc::unpack_tables)
struct UnpackTables {
    unsigned short lut[kUnpackLutEntries];
    int escape[4];
};

// Field widths of the codec parameters (the file's, with the handle's block-switching fields)
struct UnpackParams {
    int nScaleBits, nMantSizeBits, blkBitsA, blkBitsB, nShort, nLines;
};

// Band tables of the four block shapes, index (a == nShort) * 2 + (b == nShort): (L,L), (L,S), (S,L), (S,S)
struct UnpackBands {
    int nBands[4];              // < 0: no band table for the shape (chunks of it are refused)
    int halfN[4];
    const int* bandN[4];        // [nBands[s]] lines per band
};

// Where one chunk's fields go.  Null pointers are skipped.  sf / ba are written for bands [0, nBands) and zeroed on
// [nBands, padBands); the mantissas at the band's own lines [0, halfN) (zero where a band has no bits) and zeroed on
// [halfN, padLines); the M/S switch (joint ch0) like sf.
struct UnpackDst {
    int32_t* table;
    int32_t* oscale;            // non-joint: [1]; joint ch0: [4] (L, R, M, S); joint ch1: unused
    int32_t* ms;                // joint ch0 only
    int32_t* sf;
    int32_t* ba;
    int32_t* mant;
    int padBands, padLines;
};

// MSB-first reader over [p, p + nBytes): a 64-bit window, top `valid` bits are the next ones
struct UnpackBits {
    const uint8_t* p;
    int64_t nBytes, nBits, pos, next;
    uint64_t win;
    int valid;
    MRC_HD void init(const uint8_t* payload, int64_t n) {
        p = payload; nBytes = n; nBits = n * 8; pos = 0; next = 0; win = 0; valid = 0;
    }
    MRC_HD void refill() {                      // valid <= 32 on entry: 32 more bits, zeros past the payload
        uint32_t w;
        if (next + 4 <= nBytes) {
            w = (uint32_t)p[next] << 24 | (uint32_t)p[next + 1] << 16 | (uint32_t)p[next + 2] << 8 | (uint32_t)p[next + 3];
        } else {
            w = 0;
            for (int i = 0; i < 4; ++i) w = (w << 8) | (next + i < nBytes ? (uint32_t)p[next + i] : 0u);
        }
        win |= (uint64_t)w << (32 - valid);
        valid += 32;
        next += 4;
    }
    MRC_HD unsigned peek9() {
        if (valid < kUnpackPeekBits) refill();
        return (unsigned)(win >> (64 - kUnpackPeekBits));
    }
    MRC_HD void skip(int n) {                   // n <= valid (after a peek of at least n bits)
        win <<= n;
        valid -= n;
        pos += n;
    }
    // n <= 32 (every field is at most 16 bits wide); false if the read would pass the end of the payload
    MRC_HD bool get(int n, uint32_t* v) {
        if (n <= 0) { *v = 0; return true; }
        if (pos + n > nBits) return false;
        if (valid < n) refill();
        *v = (uint32_t)(win >> (64 - n));
        skip(n);
        return true;
    }
};

MRC_HD uint32_t unpack_u32le(const uint8_t* p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// The block shape of a chunk from its block-switch bits (4 bits into the payload): 0..3 as in UnpackBands.
MRC_HD int unpack_chunk_shape(const uint8_t* payload, int64_t nBytes, const UnpackParams& P, int* shape) {
    UnpackBits r;
    r.init(payload, nBytes);
    uint32_t t, a, b;
    if (!r.get(4, &t) || !r.get(P.blkBitsA, &a) || !r.get(P.blkBitsB, &b)) return kUnpackTruncated;
    *shape = (a ? 2 : 0) + (b ? 1 : 0);          // pacfileThem.py:206-207: any set bit means the short length
    return kUnpackOk;
}

// Parse one channel chunk (payload of nBytes after its length field).  joint / ch select the chunk's kind; wantShape
// >= 0 refuses a chunk of another shape.  *shapeOut = the chunk's shape.  Returns an UnpackStatus.
MRC_HD int unpack_chunk(const uint8_t* payload, int64_t nBytes, const UnpackParams& P, const UnpackBands& B,
                        const unsigned short* lut, const int* escape, int joint, int ch, int wantShape, int* shapeOut,
                        const UnpackDst& D) {
    UnpackBits r;
    r.init(payload, nBytes);
    uint32_t table, swA, swB, v;
    if (!r.get(4, &table)) return kUnpackTruncated;
    if (table != kUnpackRawTable && table > 3) return kUnpackBadTable;
    if (!r.get(P.blkBitsA, &swA) || !r.get(P.blkBitsB, &swB)) return kUnpackTruncated;
    const int shape = (swA ? 2 : 0) + (swB ? 1 : 0);
    const int nb = B.nBands[shape];
    if (nb < 0 || nb > kUnpackMaxBands || (wantShape >= 0 && shape != wantShape)) return kUnpackBadShape;
    *shapeOut = shape;
    if (D.table) *D.table = (int32_t)table;
    if (joint) {
        if (ch == 0) {
            for (int i = 0; i < 4; ++i) {
                if (!r.get(P.nScaleBits, &v)) return kUnpackTruncated;
                if (D.oscale) D.oscale[i] = (int32_t)v;
            }
            for (int i = 0; i < nb; ++i) {
                if (!r.get(1, &v)) return kUnpackTruncated;
                if (D.ms) D.ms[i] = (int32_t)v;
            }
            if (D.ms) for (int i = nb; i < D.padBands; ++i) D.ms[i] = 0;
        }
    } else {
        if (!r.get(P.nScaleBits, &v)) return kUnpackTruncated;
        if (D.oscale) D.oscale[0] = (int32_t)v;
    }
    const int* bandN = B.bandN[shape];
    const unsigned short* tlut = lut + (table & 3) * (1 << kUnpackPeekBits);
    const int esc = escape[table & 3];
    int line = 0;
    for (int band = 0; band < nb; ++band) {
        uint32_t bits, sf;
        if (!r.get(P.nMantSizeBits, &bits)) return kUnpackTruncated;
        if (bits) ++bits;
        if (bits > 16) return kUnpackBadAlloc;    // codecThem.py:292-293: the encoder never allocates more
        if (!r.get(P.nScaleBits, &sf)) return kUnpackTruncated;
        D.ba[band] = (int32_t)bits;
        D.sf[band] = (int32_t)sf;
        const int n = bandN[band];
        int32_t* m = D.mant + line;
        if (!bits) {
            for (int j = 0; j < n; ++j) m[j] = 0;
        } else if (table == kUnpackRawTable) {
            for (int j = 0; j < n; ++j) {
                if (!r.get((int)bits, &v)) return kUnpackTruncated;
                m[j] = (int32_t)v;
            }
        } else {
            for (int j = 0; j < n; ++j) {
                const unsigned e = tlut[r.peek9()];
                const int len = (int)(e >> 8);
                if (!len) return kUnpackBadCode;
                if (r.pos + len > r.nBits) return kUnpackTruncated;
                r.skip(len);
                int val = (int)(e & 0xffu);
                if (val == esc) {
                    if (!r.get((int)bits, &v)) return kUnpackTruncated;
                    val = (int)v;
                }
                m[j] = (int32_t)val;
            }
        }
        line += n;
    }
    for (int i = nb; i < D.padBands; ++i) { D.ba[i] = 0; D.sf[i] = 0; }
    for (int i = line; i < D.padLines; ++i) D.mant[i] = 0;
    return kUnpackOk;
}

// Validated payload of chunk `off` in buf[0, len): false unless the length field and the payload lie inside.
MRC_HD bool unpack_locate(const uint8_t* buf, int64_t len, int64_t off, const uint8_t** payload, int64_t* nBytes) {
    if (off < 0 || len < 4 || off > len - 4) return false;
    const int64_t n = (int64_t)unpack_u32le(buf + off);
    if (n > len - off - 4) return false;
    *payload = buf + off + 4;
    *nBytes = n;
    return true;
}

// Outputs of the fixed-stride layout of mrc_unpack_blocks (include/mrc_hip.h)
struct UnpackFixedOut {
    int32_t *a, *b, *table, *oscale, *ms, *sf, *ba, *mant;
};

// Chunk ch of block blk in the layout of mrc_unpack_blocks: the same checks as the host parser, the block's first chunk
// giving the shape its second must have (read again from that chunk's block-switch bits: chunks parse independently).
MRC_HD int unpack_fixed_chunk(const uint8_t* buf, int64_t len, const int64_t* chunkOffset, int64_t blk, int ch, int nch,
                              int joint, const UnpackParams& P, const UnpackBands& B, const unsigned short* lut,
                              const int* escape, const UnpackFixedOut& O) {
    const int64_t c = blk * nch + ch;
    const uint8_t* payload;
    int64_t nBytes;
    if (!unpack_locate(buf, len, chunkOffset[c], &payload, &nBytes)) return kUnpackTruncated;
    int want = -1;
    if (ch > 0) {
        const uint8_t* p0;
        int64_t n0;
        if (!unpack_locate(buf, len, chunkOffset[blk * nch], &p0, &n0) || unpack_chunk_shape(p0, n0, P, &want) != kUnpackOk)
            return kUnpackTruncated;              // (the first chunk's own lane reports it as well)
    }
    UnpackDst D;
    D.table = O.table + c;
    D.oscale = joint ? (ch == 0 ? O.oscale + blk * 4 : nullptr) : O.oscale + c;
    D.ms = joint && ch == 0 ? O.ms + blk * kUnpackMaxBands : nullptr;
    D.sf = O.sf + c * kUnpackMaxBands;
    D.ba = O.ba + c * kUnpackMaxBands;
    D.mant = O.mant + c * (int64_t)P.nLines;
    D.padBands = kUnpackMaxBands;
    D.padLines = P.nLines;
    int shape = 0;
    const int rc = unpack_chunk(payload, nBytes, P, B, lut, escape, joint, ch, want, &shape, D);
    if (rc != kUnpackOk) return rc;
    if (ch == 0) {
        O.a[blk] = (shape & 2) ? P.nShort : P.nLines;
        O.b[blk] = (shape & 1) ? P.nShort : P.nLines;
    }
    return kUnpackOk;
}

}  // namespace mrc
