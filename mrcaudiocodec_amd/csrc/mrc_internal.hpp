// Internal declarations shared by the host glue (mrc_api.cpp, mrc_tables.cpp) and the gfx950
// kernels (mrc_kernels.hip).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>
#include "mrc_hip.h"
#include "mrc_unpack.hpp"

namespace mrc {

constexpr int kMaxRadices = 8;
// how a channel's samples are held: float64 signed fractions (what pcmfile.py:98 hands the codec) or the file's
// int16 PCM codes, converted on load (dev::pcm16_to_frac)
constexpr int kSampleF64 = MRC_SAMPLES_F64, kSampleI16 = MRC_SAMPLES_PCM16;
constexpr int kMaxBands = MRC_MAX_BANDS;

// Everything a kernel needs to know about one block shape (a,b).  POD, passed by value; the
// pointers address one device blob owned by the handle.
struct LineConstants { double z, quiet, lowE; int band, pad; };      // 32 bytes: two 16-byte loads per line

struct DevShape {
    int a, b, N, halfN, Q, H;        // N = a+b, halfN = N/2 lines, Q = N/4 (MDCT FFT), H = N/2 (psycho FFT)
    int shift;                       // (b-a)/4: signed circular shift that maps n0=(b+1)/2 to the standard phase
    int nBands;
    int peakLast;                    // N/2 - 100 (psychoac.py:160)
    int nRadQ, nRadH;
    int radQ[kMaxRadices], radH[kMaxRadices];
    int nScaleBits, maxMantBits;
    double twoOverN;                 // 2.0/N (mdct.py:76)
    double binHz;                    // py2 integer sampleRate/N (psychoac.py:165)
    double xiDen;                    // (N**2.)*(3./8.) (psychoac.py:151)
    double budgetMono;               // codecThem.py:299-306 (reservoir added last)
    double budgetJointPre;           // codecThem.py:381-388 (before `+= bitReservoir`)
    double blkswA, blkswB;
    const double* win;               // [N] transition window (window.py:104-121)
    int winSymmetric;                // win[n] == win[N - 1 - n] bit for bit (true for a = b)
    const double* hann;              // [N] window.py:28-45
    const double2* pre;              // [Q] exp(-i pi (4n+1)/(4M)), M = N/2
    // [halfN] zb, quiet, lowE and the band of a line side by side (smr_kernel's sweep).  Between two pointers that smr_kernel
    // does not read: next to loLine / hiLine / linesPerHz the compiler fetched the four with one 32-byte scalar load for the masker
    // table and kept -- and, at its scalar-register limit, reloaded from a spill lane in every chunk -- all eight registers for
    // the sake of this one pointer.
    const struct LineConstants* lineC;
    const double2* post;             // [Q] exp(-i pi k / M)
    const double2* wQ;               // [Q] exp(-2 pi i t/Q)
    const double2* wH;               // [H] exp(-2 pi i t/H)
    const double2* wN;               // [H] exp(-2 pi i k/N)
    const double2* fftTw;            // H = 1024 only: per-pass twiddles of the psycho FFT (dev::fft_regs_1024), else null
    const double* zb;                // [halfN] Bark(MDCTFreq) (psychoac.py:27-29,142-143)
    const double* quiet;             // [halfN] Intensity(Thresh(MDCTFreq)) (psychoac.py:155)
    const double* lowE;              // [halfN] 2^(2.7 log2(10) (zb+1/2)): per-line factor of the -27 dB/Bark lower slope
    const int* bandLo;               // [nBands]
    const int* bandN;                // [nBands]
    const unsigned char* bandOfLine; // [halfN]
    const unsigned short* loLine;    // [halfN] first line j with zb[j] - zb[k] >= -1/2 (search hint)
    const unsigned short* hiLine;    // [halfN] first line j with zb[j] - zb[k] > 1/2, halfN if none (search hint)
    double linesPerHz;               // N / sampleRate
    // NumPy's pairwise summation of every band's lines as a static tree (ms_plan): msLeaves (lo, n) runs of <= 128
    // lines, then internal nodes (left, right) in an order where children come first, then the root node of each band
    const int* msPlan;               // [2 msLeaves + 2 msInternal + nBands]
    int msLeaves, msInternal;
};

// one device allocation, freed with its owner (the rule for every owning type: mrc_handle.hpp)
struct DevFree { void operator()(void* p) const { (void)hipFree(p); } };
using DevPtr = std::unique_ptr<void, DevFree>;

struct HostShape {
    DevShape dev{};                  // device view (pointers valid on the device)
    std::vector<int> bandN, bandLo;  // host copies
    DevPtr blob;                     // device allocation backing dev.*
};

// mrc_tables.cpp
bool band_table(const mrc_config& cfg, int a, int b, std::vector<int>* count);   // host only
std::string band_table_error(const mrc_config& cfg, int a, int b);                 // why band_table refused
// error text of the last failed call that has no handle (mrc_create, mrc_band_table, mrc_pac_header, mrc_pac_read_header)
std::string& create_error();
// The summation tree np.sum walks over each band's contiguous run of lines (pairwise summation: runs of more than 128
// elements are halved, the first half rounded down to a multiple of 8).  -> plan laid out as DevShape::msPlan.
void ms_plan(const std::vector<int>& bandLo, const std::vector<int>& bandN, std::vector<int>* plan, int* nLeaves,
             int* nInternal);
bool build_shape(const mrc_config& cfg, int a, int b, HostShape* out, std::string* err);
// Synthesis only: the fields decode_kernel reads of a shape (a, b, N, halfN, Q, shift, radQ / nRadQ / wQ, pre / post, win),
// by build_shape's own expressions, and nothing else -- no band table, no masking model, so no lower limit on the length.
// The rule is the transform's: a, b > 0, a + b and b - a divisible by 4, N/4 and N/2 products of 2s and 3s.
bool synth_shape_rule(int a, int b, std::string* err);                              // host only
bool build_synth_shape(int a, int b, HostShape* out, std::string* err);
// the bit budgets of a block of shape (a, b) with nb bands at target_bits_per_sample tbps (codecThem.py:299-306 mono,
// 381-388 joint before the reservoir is added): the one copy of the float arithmetic the shape tables and the rate ladder share
void shape_budgets(const mrc_config& cfg, double tbps, int a, int b, int nb, double* budgetMono, double* budgetJointPre);
int scale_factor_host(double v, int nScaleBits, int nMantBits);

// mrc_kernels.hip -- launchers (enqueue only)
hipError_t launch_mdct(const DevShape& S, int64_t nFrames, const void* chL, const void* chR, int fmt,
                       int64_t stride, const int64_t* offsets, bool applyWindow, double* lines, int* oscale,
                       hipStream_t st);
size_t mdct_generic_lds_bytes(const DevShape& S);   // dynamic LDS of mdct_kernel (and decode_kernel) for shape S
// mrc_kernels_long.hip -- long-block specialisation (a = b = 1024)
bool mdct_long_applicable(const DevShape& S, int64_t stride, const int64_t* offsets, const void* chL,
                          const void* chR, int fmt);
hipError_t launch_mdct_long(const DevShape& S, int64_t nFrames, const void* chL, const void* chR, int fmt,
                            int64_t stride, const int64_t* offsets, double* lines, int* oscale, hipStream_t st);
hipError_t launch_window(const DevShape& S, int64_t nBlocks, const double* in, double* out, hipStream_t st);
hipError_t launch_unscale(int64_t nBlocks, int halfN, const double* scaled, const int* oscale, double* lines,
                          hipStream_t st);
size_t smr_generic_lds_bytes(const DevShape& S);    // dynamic LDS of smr_kernel for shape S
bool smr_peaks_fit(const DevShape& S);              // can smr_kernel hold every peak a block of shape S may have?
hipError_t launch_smr(const DevShape& S, int64_t nFrames, const void* chL, const void* chR, int fmt,
                      int64_t stride, const int64_t* offsets, const double* lines, const int* oscale,
                      double* smr, double* thresh, double* bandPeak /* [frames*signals][nBands] or null */,
                      const int* msSwitch /* joint: [frames][nBands] -> only the SMRs the encoder uses are computed; null: all */,
                      bool exactSpread, hipStream_t st,
                      unsigned long long* sens = nullptr /* MRC_OPT_SENSITIVITY: counters [MRC_SENS_COUNT] on the device */);
// launch_smr's other unit: the mono long block (mrc_kernels_smr_mono.hip)
hipError_t launch_smr_mono_long(const DevShape& S, int64_t nFrames, const void* chL, int fmt, int64_t stride,
                                const int64_t* offsets, const double* lines, const int* oscale, double* smr,
                                double* bandPeak, hipStream_t st, unsigned long long* sens);
// mrc_kernels_probe.hip: one __device__ helper on the caller's words (mrc_dev_helper_probe).  probe_words: the words per element
// of the three inputs and the output, false for an unknown probe
bool probe_words(int probe, int* w0, int* w1, int* w2, int* wout);
hipError_t launch_probe(int probe, const void* in0, const void* in1, const void* in2, void* out, int n, int threads,
                        hipStream_t st);
// mrc_kernels_sens.hip: decisions within a guard band of rounding (quantiser edges, allocation ties, M/S threshold)
hipError_t launch_sensitivity(const DevShape& S, int64_t nFrames, int joint, const double* lines, const int* oscale,
                              const double* smr, const double* bandPeak, const int* msSwitch, const int* bitAlloc,
                              const int* scaleFactor, unsigned long long* sens, unsigned char* frameFlags, hipStream_t st);
hipError_t launch_alloc_quant(const DevShape& S, int64_t nFrames, int joint, const double* lines,
                              const int* oscale, const double* smr, const int* resIn, int* msSwitch,
                              int* bitAlloc, int* scaleFactor, void* mantissa, int mantFmt /* MRC_MANTISSA_* */,
                              int* resOut, double* bandPeakWs,
                              bool peaksReady /* bandPeakWs already filled by launch_smr */,
                              bool msReady /* msSwitch already filled (launch_ms_switch ran before launch_smr) */,
                              hipEvent_t evStats, hipEvent_t evAlloc /* recorded after band_stats / after bitalloc (in front of the fused
                              long-block kernel); null: not */,
                              hipStream_t st);
hipError_t launch_pcm_to_float(int64_t n, const short* pcm, double* out, hipStream_t st);
hipError_t launch_quantize_uniform(int64_t n, int nBits, const double* x, long long* out, hipStream_t st);
hipError_t launch_bark(int64_t n, const double* f, double* out, hipStream_t st);
size_t alloc_workspace_bytes(const DevShape& S, int64_t nFrames, int joint);   // bandPeakWs size
// band_stats_kernel alone: bandPeak [n][nsig][nBands] = max |line| of every band of every signal (what the stage entry points
// have in place of smr_kernel's peaks)
hipError_t launch_band_peaks(const DevShape& S, int64_t nFrames, int joint, const double* lines, double* bandPeak,
                             hipStream_t st);
// mrc_kernels_decode.hip
hipError_t launch_decode(const DevShape& S, int64_t nBlocks, int nStreams, const int* oscale, const int* msSwitch,
                         const int* scaleFactor, const int* bitAlloc, const int* mantissa, const int64_t* outOffset,
                         double* outL, double* outR, hipStream_t st);
hipError_t launch_pcm16(int64_t n, const double* x, short* out, hipStream_t st);
// launch_decode at a reduced sample rate: the parsed arrays, bands and line stride are those of the block's FULL shape F,
// of which the first R.halfN lines are dequantised; the inverse transform, window and overlap-add are R's (a synthesis
// shape, build_synth_shape, of F's (a, b) / D), and outOffset counts reduced samples
hipError_t launch_decode_reduced(const DevShape& F, const DevShape& R, int64_t nBlocks, int nStreams, const int* oscale,
                                 const int* msSwitch, const int* scaleFactor, const int* bitAlloc, const int* mantissa,
                                 const int64_t* outOffset, double* outL, double* outR, hipStream_t st);
// One output plane per block instead of one per channel (mrc_pac_store_decode_window_mix): one workgroup per joint slot
// writes its L (mixSel 0), R (1) or mid (L + R) / 2 (2; formed on the lines, decode_line_mid).  A non-joint group holds
// nPairs pairs of slots first -- slots 2 w, 2 w + 1 are the two channels of a stereo file's last block, workgroup w writes
// their mid -- and single slots after them, nWorkgroups - nPairs of them, each written as it is.  R: the reduced shape of
// launch_decode_reduced, null at full rate.  outOffset [nWorkgroups]: per workgroup, not per slot.
hipError_t launch_decode_mix(const DevShape& F, const DevShape* R, int64_t nWorkgroups, int joint, int mixSel, int64_t nPairs,
                             const int* oscale, const int* msSwitch, const int* scaleFactor, const int* bitAlloc,
                             const int* mantissa, const int64_t* outOffset, double* out, hipStream_t st);
// launch_decode (R null) / launch_decode_reduced and launch_decode_mix with one band gain per line between the dequantiser
// and the inverse transform (mrc_pac_store_decode_window_shaped): line k of a block is multiplied once by
// gain[unit[i]][lineBand[k]] unless lineBand[k] is kNoLineBand.  lineBand [F.halfN] counts the lines of the FULL shape at every
// rate; unit is indexed as outOffset is (per slot, per workgroup); all three DEVICE.
constexpr unsigned short kNoLineBand = 0xffff;      // lineBand: the line lies in no band
hipError_t launch_decode_shaped(const DevShape& F, const DevShape* R, const unsigned short* lineBand, const double* gain,
                                const int* unit, int nBands, int64_t nBlocks, int nStreams, const int* oscale, const int* msSwitch,
                                const int* scaleFactor, const int* bitAlloc, const int* mantissa, const int64_t* outOffset,
                                double* outL, double* outR, hipStream_t st);
hipError_t launch_decode_shaped_mix(const DevShape& F, const DevShape* R, const unsigned short* lineBand, const double* gain,
                                    const int* unit, int nBands, int64_t nWorkgroups, int joint, int mixSel, int64_t nPairs,
                                    const int* oscale, const int* msSwitch, const int* scaleFactor, const int* bitAlloc,
                                    const int* mantissa, const int64_t* outOffset, double* out, hipStream_t st);
// mrc_kernels_pack.hip -- `.pac` chunk packing on the device
constexpr int kPackLutSize = 65;     // the largest value in any Huffman table is 64
constexpr int kPackRawTable = 15;    // codecThem.py:149
struct PackTables {                  // mrc_pack.cpp: pack_tables()
    // per table and value (last index: any other value): code | length << 16 | 1 << 31 where the raw mantissa follows
    unsigned emit[4 * (kPackLutSize + 1)];
    int escape[4];
};
struct PackParams {
    int nch, joint, useHuffman;
    int nScaleBits, nMantSizeBits, blkBitsA, blkBitsB;      // field widths
    unsigned bitA, bitB;                                    // block-switching bits of this shape (pacfileThem.py:720-723)
};
void pack_tables(PackTables* out);                          // host (mrc_pack.cpp), from mrc_huffman_tables.hpp
size_t pack_workspace_bytes(int64_t nChunks);
hipError_t launch_pack(const DevShape& S, const PackParams& P, const PackTables& T, int64_t nBlocks, const int* oscale,
                       const int* msSwitch, const int* scaleFactor, const int* bitAlloc, const void* mant, int mantFmt,
                       const int* tableIn /* nullable */, int* tableOut, int* bitsSaved /* nullable */, unsigned char* out,
                       long long outCap, long long* blockOffset /* [nBlocks + 1] */, void* ws /* pack_workspace_bytes */,
                       int boundBytes /* largest chunk payload */, bool allBandsNonEmpty /* of this shape's table */,
                       hipStream_t st);
// The three steps of launch_pack on their own, for chunks that several shape groups contribute to ONE output in a
// given order (the chained stream encode): chunkMap [nBlocks * nch] (nullable) = where each of this group's chunks sits
// in the global chunk order; chunkBytes / pos are indexed by that global index.  chunkStream (nullable) [nChunks]:
// the stream each global chunk belongs to -- every stream's first chunk is preceded by a header of hdrLen bytes.
struct PackWs {                      // views into a workspace of pack_workspace_bytes(nChunks)
    long long* pos; long long* tileSum; long long* total; int* errorFlag; int* chunkBytes;
};
PackWs pack_ws_views(void* ws, int64_t nChunks);
hipError_t launch_pack_plan(const DevShape& S, const PackParams& P, const PackTables& T, int64_t nBlocks,
                            const int* bitAlloc, const void* mant, int mantFmt, const int* tableIn, int* tableOut,
                            int* bitsSaved, const PackWs& W, const long long* chunkMap, bool allBandsNonEmpty,
                            hipStream_t st);
hipError_t launch_pack_scan(int64_t nChunks, int nch /* 0: no block offsets */, const PackWs& W, long long* blockOffset,
                            const int* chunkStream, int hdrLen, hipStream_t st);
hipError_t launch_pack_write(const DevShape& S, const PackParams& P, const PackTables& T, int64_t nBlocks,
                             const int* oscale, const int* msSwitch, const int* scaleFactor, const int* bitAlloc,
                             const void* mant, int mantFmt, const int* table, const PackWs& W, const long long* chunkMap,
                             unsigned char* out, long long outCap, int boundBytes, bool allBandsNonEmpty, hipStream_t st);
hipError_t launch_pack_export(const void* ws, int64_t nChunks, long long* hostOut /* page-locked: {total, error flag} */,
                              hipStream_t st);
const int* pack_error_flag(const void* ws, int64_t nChunks);          // device addresses inside ws
const long long* pack_total_bytes(const void* ws, int64_t nChunks);
// mrc_kernels_unpack.hip -- `.pac` chunk parsing on the device (the parser itself: mrc_unpack.hpp)
void unpack_tables(UnpackTables* out);                      // host (mrc_pack.cpp), from mrc_huffman_tables.hpp
const char* unpack_status_text(int flag);                   // the words for a set of (1 << UnpackStatus) bits (mrc_api_decode.cpp)
struct UnpackErr { int flag; int firstBad; };               // first bad chunk (lowest index) and its UnpackStatus
// layout of mrc_unpack_blocks: chunk c = blk * nch + ch, buf / chunkOffset / outputs in device memory
hipError_t launch_unpack_fixed(const UnpackParams& P, const UnpackBands& B, const UnpackTables* T /* device */,
                               int64_t nBlocks, int nch, int joint, const uint8_t* buf, int64_t len,
                               const int64_t* chunkOffset, const UnpackFixedOut& O, UnpackErr* err, hipStream_t st);
// dense per-(shape, kind) group arrays that launch_decode consumes, at slots the host plan assigns
constexpr int kUnpackGroups = 8;     // (shape 0..3) x (joint, non-joint): group = shape * 2 + (non-joint)
struct UnpackGroupDev {
    int shape, joint, nb, halfN;
    int* oscale;                     // [n][joint ? 4 : 1]
    int* ms;                         // [n][nb] (joint)
    int* sf;                         // [n][joint ? 2 : 1][nb]
    int* ba;
    int* mant;                       // [n][joint ? 2 : 1][halfN]
};
struct UnpackPlanEntry { long long off; int groupStream; int slot; };   // groupStream = group * 2 + stream (joint ch)
hipError_t launch_unpack_dense(const UnpackParams& P, const UnpackBands& B, const UnpackTables* T, int64_t nChunks,
                               const UnpackPlanEntry* plan, const uint8_t* buf, int64_t len,
                               const UnpackGroupDev* groups /* device [kUnpackGroups] */, UnpackErr* err, hipStream_t st);
// decoded planes -> WAV-order interleaved int16 per file, the first skip samples of each file dropped: file f's values
// are [outStart[f], outStart[f + 1]), its channel c at x[c * planeStride + xStart[f] + skip + t]
hipError_t launch_pcm16_interleave(int64_t nFiles, int64_t nOut, const long long* outStart, const long long* xStart,
                                   const int* nch, int skip, const double* x, int64_t planeStride, short* out,
                                   hipStream_t st);
// mrc_kernels_nmr.hip -- noise-to-mask ratio of decoded blocks against their source (mrc_pac_nmr)
struct NmrPlane { long long dst, src, frames, len; };   // padded plane: out[dst + t], t < len; samples src[src + t - L]
struct NmrEntry {                    // one (block, channel) of a file, all of one block shape per launch
    long long out;                   // entry index: row of the band arrays and of stat
    long long ana;                   // row of the shape's source analysis (X, T)
    int group, slot, ch, b;          // parsed chunk(s): UnpackGroupDev group and slot; output channel; new samples b
};
hipError_t launch_nmr_pad(int64_t nPlanes, const NmrPlane* planes /* device */, int64_t maxLen, int L, const short* src,
                          short* out, hipStream_t st);
// bandNoise / bandMask: [entries][kMaxBands] or null; stat [entries][2]: max_j r_j, b * mean_j r_j
hipError_t launch_nmr_band(const DevShape& S, int64_t nEntries, const NmrEntry* entries, const UnpackGroupDev* groups,
                           const double* lines, const double* thresh, double* bandNoise, double* bandMask, double* stat,
                           hipStream_t st);
// fileOut [nFiles][4]: max r, sum of b * mean r, disturbed blocks, 0.  File f's entries: [entryStart[f], entryStart[f + 1])
hipError_t launch_nmr_file(int64_t nFiles, const long long* entryStart, const int* nch, const double* stat, double* fileOut,
                           hipStream_t st);
// mrc_kernels_store.hip -- windows of resident `.pac` files (mrc_pac_store_decode_window)
struct WindowItem {                  // one item of a slab
    long long plane;                 // where its first decoded channel's plane starts in the slab's planes (doubles)
    long long start;                 // the window's first sample, in the coordinates of mrc_decode_pac_pcm16's output (divided
                                     // by the rate divisor: mrc_pac_store_decode_window_reduced)
    long long nSamples;              // the file's length in those coordinates; 0: the item needs no block, its plane is not read
    int nch, pad_;                   // decoded channels: planes at plane + c * (window + 4 L)
};
// out [nItems][nchOut][window] in `format` (MRC_WINDOW_*) <- planes[item.plane + c * (window + 4 L) + 2 L + t], zero where
// start + t lies outside [0, nSamples); a one-channel item fills every output channel.  (L: the planes' margin unit --
// n_mdct_lines, divided by the rate divisor where there is one.)
hipError_t launch_window_out(int64_t nItems, const WindowItem* items /* device */, int64_t window, int nchOut, int format,
                             int L, const double* planes, void* out, hipStream_t st);
// mrc_pac_store_decode_window_resampled: out [nItems][nchOut][window] <- the polyphase fold of the items' planes, which hold
// INTERMEDIATE samples (item.start, item.nSamples in those; planes of planeLen doubles, sample m at 2 L + m - item.start).
// Output t of item k is output sample n = outStart[k] + t; taps (device) [2 W][up]; evenOdd, skew: the LDS layout
// (resample_lds_layout).  Refuses a run of more than 4089 intermediate samples per 256 outputs.
hipError_t launch_resample_out(int64_t nItems, const WindowItem* items /* device */, const long long* outStart /* device */,
                               int64_t window, int nchOut, int format, int L, int64_t planeLen, int up, int down, int W,
                               int evenOdd, int skew, const double* taps, const double* planes, void* out, hipStream_t st);
// mrc_pac_store_decode_window_sum: one term of an item, the planning unit of that call -- the WindowItem of the other calls,
// the factor its signal is multiplied by and, when the call resamples, its first OUTPUT sample (else 0).
struct SumTerm {
    WindowItem w;
    double gain;
    long long outStart;
};
// out [nRows][nchOut][window] in `format` <- the left fold from +0.0, over terms [termOffset[i], termOffset[i + 1]) of item i in
// that order, of gain * (window_out_kernel's value of the term): every product rounded once, then added.  An item without
// terms is +0.0.  terms, termOffset [nRows + 1]: device.
hipError_t launch_sum_out(int64_t nRows, const SumTerm* terms, const long long* termOffset, int64_t window, int nchOut,
                          int format, int L, const double* planes, void* out, hipStream_t st);
// ... and the same fold of gain * (resample_out_kernel's value of the term, output t at output sample term.outStart + t)
hipError_t launch_resample_sum_out(int64_t nRows, const SumTerm* terms, const long long* termOffset, int64_t window, int nchOut,
                                   int format, int L, int64_t planeLen, int up, int down, int W, int evenOdd, int skew,
                                   const double* taps, const double* planes, void* out, hipStream_t st);
// mrc_pac_store_decode_window_speeds: one ratio of the call's list as resample_multi_sum_out_kernel reads it.  W == 0: the
// unit ratio -- no filter, the term's value is sum_out_kernel's.  Else up / down reduced, the half width, the run's LDS layout
// under the natural lane map (skew: the better of resample_lds_cycles(up, down, 1, 0 | 1)) and the taps (device) [2 W][up].
struct SpeedRatio {
    int up, down, W, skew;
    const double* taps;
};
// ... the same fold with the ratio read per term: term j is read at ratios[ratioOf[j]] (ratioOf [terms], ratios [nRatios]:
// device; ratiosHost: the same records on the host, for the check of the run that the other resampling launchers make).
// A term of a non-unit ratio keeps its planes as launch_resample_sum_out's terms do, one of the unit ratio as
// launch_sum_out's; both kinds at the one planeLen.
hipError_t launch_resample_multi_sum_out(int64_t nRows, const SumTerm* terms, const int* ratioOf, const SpeedRatio* ratios,
                                         const SpeedRatio* ratiosHost, int nRatios, const long long* termOffset, int64_t window,
                                         int nchOut, int format, int L, int64_t planeLen, const double* planes, void* out,
                                         hipStream_t st);
// mrc_pac_store_decode_window_spans: the audible part of one term, a record beside its SumTerm (which keeps its layout).  The
// term sounds at row samples first <= t < first + len and is silent elsewhere; with j = t - first its value is e * v, e =
// (2 j + 1) / (2 fadeIn) where j < fadeIn, (2 (len - 1 - j) + 1) / (2 fadeOut) where j >= len - fadeOut, else v itself
// (fadeIn + fadeOut <= len: one ramp at most).  The term's planes were planned for [first, first + len) cut to the row, NOT
// for the row: a term of the unit ratio keeps row sample t at plane[2 L + t - origin] and SumTerm::w.start is the file's
// sample at row sample `origin`; a resampled term keeps its intermediate samples as ever (w.start the first of them).
struct TermSpan {
    long long first, len, fadeIn, fadeOut, origin;
};
// launch_sum_out, launch_resample_sum_out and launch_resample_multi_sum_out over terms with spans (spans [terms]: device).
// Planes of planeLen doubles in all three.  A sample outside a term's span is never read from its plane.
hipError_t launch_span_sum_out(int64_t nRows, const SumTerm* terms, const TermSpan* spans, const long long* termOffset,
                               int64_t window, int nchOut, int format, int L, int64_t planeLen, const double* planes, void* out,
                               hipStream_t st);
hipError_t launch_span_resample_sum_out(int64_t nRows, const SumTerm* terms, const TermSpan* spans, const long long* termOffset,
                                        int64_t window, int nchOut, int format, int L, int64_t planeLen, int up, int down, int W,
                                        int evenOdd, int skew, const double* taps, const double* planes, void* out, hipStream_t st);
hipError_t launch_span_resample_multi_sum_out(int64_t nRows, const SumTerm* terms, const TermSpan* spans, const int* ratioOf,
                                              const SpeedRatio* ratios, const SpeedRatio* ratiosHost, int nRatios,
                                              const long long* termOffset, int64_t window, int nchOut, int format, int L,
                                              int64_t planeLen, const double* planes, void* out, hipStream_t st);
// mrc_pac_store_decode_window_reverb (mrc_kernels_reverb.hip): overlap-save at a hop of B = MRC_STORE_REVERB_BLOCK samples and
// transforms of N = 2 B points.  A source of forward transforms: sample i < take of segment seg < nSeg is g = first + seg B + i,
// its value samples[re + g] + i samples[im + g] (im < 0: no imaginary part) where lo <= g < hi and zero elsewhere; the
// segment's N bins go to spectra[(spec + seg) N ..).  A term's dry signal (take = N) and a response of the bank, whose
// segments are its partitions of B taps (take = B), are both sources.
struct ReverbSource {
    long long re, im, first, lo, hi, spec;
    int nSeg, take;
};
// sources, samples, twiddle (the first quadrant of exp(-2 pi i t / N), N / 4 values), spectra: device
hipError_t launch_reverb_forward(int64_t nSources, int64_t maxSeg /* the largest nSeg */, const ReverbSource* sources,
                                 const double* samples, const double2* twiddle, double2* spectra, hipStream_t st);
// One term of a row: its dry samples of channel c at dry[dry + c chStride + t], t counted from the term's window start; spec < 0:
// not convolved, else the term's first spectrum (segment s = -(nPart - 1), segment s at spec + s + nPart - 1) and ir, the
// first of the response's nPart partitions in the bank.
struct ReverbTerm {
    long long dry, spec, ir;
    int nPart, pad_;
    double gain;
};
// out [nRows][nchOut][window] in `format` <- the left fold from +0.0, over terms [termOffset[i], termOffset[i + 1]) of row i in
// that order, of gain * (the dry sample | the term's convolution with its response), every product rounded once, then added.
hipError_t launch_reverb_fold(int64_t nRows, const ReverbTerm* terms /* device */, const long long* termOffset /* device */,
                              int64_t window, int nchOut, int format, int64_t chStride, const double* dry, const double2* spectra,
                              const double2* bank, const double2* twiddle, void* out, hipStream_t st);
// mrc_pac_store_decode_window_routed: a term has one dry channel and a route per output channel, routes [term][nChannels], each a
// ReverbTerm whose spec is kRouteNone (no contribution), kRouteDry, or the first spectrum of the term's source of that
// response's length (routes of one length share a source); .dry is the term's dry channel in every record.
// out [nRows][nChannels][window]: channel c is launch_reverb_fold's one-channel row over the routes to c that are not absent,
// bit for bit.  One workgroup per (row, output block, group of `group` channels: 1 or 2); a channel's bits do not depend on
// the group.
constexpr long long kRouteDry = -1, kRouteNone = -2;
inline int64_t reverb_route_groups(int nChannels, int group) { return (nChannels + group - 1) / group; }
hipError_t launch_reverb_route_fold(int64_t nRows, const ReverbTerm* routes /* device */, const long long* termOffset /* device */,
                                    int64_t window, int nChannels, int group, int format, const double* dry, const double2* spectra,
                                    const double2* bank, const double2* twiddle, void* out, hipStream_t st);
// mrc_pac_store_stft_window (mrc_kernels_stft.hip).  rows (device) float64 [nRows][nch][L], L = (nFrames - 1) hop + nFft;
// win (device) [nFft]; tw (device) exp(-2 pi i t / nFft) for 0 <= t < nFft; radices: the passes of the nFft / 2 point complex
// transform, four bits each from the lowest (stft_radices); mode MRC_STFT_*, format MRC_WINDOW_F32 | _F64.  MRC_STFT_BANK:
// bankTab (device) int32 [3][nFilters] -- lo, hi, and the offset of filter q's weights in bankW (device), whose entry
// offset + (k - lo) is bin k's weight.  out [nRows][nch][nFft / 2 + 1 | nFilters][nFrames] ([2] under MRC_STFT_COMPLEX).
struct StftParams {
    const double* rows;
    const double* win;
    const double2* tw;
    const int* bankTab;
    const double* bankW;
    void* out;
    long long L, nFrames, hop;
    unsigned long long radices;
    int nRows, nch, nFft, nRad, mode, format, nFilters;
};
// 0 where n is not 2^a 3^b 5^c or takes more than 16 passes; else the radices, fours first, then 2, 3 and 5; *nRad their number
unsigned long long stft_radices(int n, int* nRad);
hipError_t launch_stft(const StftParams& P, hipStream_t st);
// One entry of mrc_pac_store_block_energy: a channel of a block, or its mid.  sel 0 / 1: output channel L / R of a joint
// slot (a non-joint slot has one channel, itself: 0); kEnergyMid: the mid (L + R) / 2 on the lines -- of a joint slot, or of
// the PAIR of non-joint slots slot, slot + 1 (a stereo file's last block).
constexpr int kEnergyMid = 2;
struct EnergyEntry { long long out; int slot, sel; };   // out: where its energy goes
hipError_t launch_block_energy(const DevShape& F, int D, int joint, int64_t nEntries, const EnergyEntry* entries /* device */,
                               const int* oscale, const int* msSwitch, const int* scaleFactor, const int* bitAlloc,
                               const int* mantissa, double* energy, hipStream_t st);
// mrc_pac_store_band_energy_window.  band_energy_kernel: B[entry.out][q] = the sum of the squares of the entry's decoded
// lines lineLo[q] <= k < lineLo[q + 1], a left fold from +0.0 in ascending k (entries as launch_block_energy's; lineLo
// (device) [nBands + 1], the shape's table of mrc_band_line_ranges).
hipError_t launch_band_energy(const DevShape& F, int joint, int nBands, const int* lineLo /* device */, int64_t nEntries,
                              const EnergyEntry* entries /* device */, const int* oscale, const int* msSwitch,
                              const int* scaleFactor, const int* bitAlloc, const int* mantissa, double* bandSums, hipStream_t st);
// mrc_pac_store_filterbank_window.  filterbank_energy_kernel: F[entry.out][q] = the left fold from +0.0 over k = lo[q] ..
// hi[q] - 1 ascending of w * x^[k]^2, the square and the product each rounded once (entries as launch_block_energy's; tab
// (device) int32 [3][nFilters]: the shape's lo, hi and the offset of each filter's row in weight (device), whose entry
// offset + (k - lo) is line k's weight -- mrc_filterbank_line_weights' rows; hi <= F.halfN).
hipError_t launch_filterbank_energy(const DevShape& F, int joint, int nFilters, const int* tab /* device */,
                                    const double* weight /* device */, int64_t nEntries, const EnergyEntry* entries /* device */,
                                    const int* oscale, const int* msSwitch, const int* scaleFactor, const int* bitAlloc,
                                    const int* mantissa, double* filterSums, hipStream_t st);
// One item of band_frames_kernel: its needed blocks are tiles [edge[edge0 + t], edge[edge0 + t + 1]), t < nTiles, in DOUBLED
// output samples, ascending and abutting; tile t's band sums of decoded channel c are row row0 + t * nch + c of B.  lo and
// hi: output samples at or before the first and at or behind the last tile edge -- a frame's ends are clamped to them
// before they are doubled, which changes no overlap and keeps every start, however extreme, inside 64 bits.
struct BandItem { long long edge0, row0, start, lo, hi; int nTiles, nch; };
// out [nItems][nchOut][nBands][nFrames] (MRC_WINDOW_F32 / _F64) <- frame j = [start + j hop, start + (j + 1) hop): the left
// fold from +0.0 over the item's tiles in ascending order, of (double)(doubled overlap) * B, where the overlap is positive
hipError_t launch_band_frames(int64_t nItems, const BandItem* items /* device */, const long long* edges /* device */,
                              int64_t nFrames, int64_t hop, int nBands, int nchOut, int format, const double* bandSums,
                              void* out, hipStream_t st);
// mrc_kernels_chain.hip -- chained stream encode: reservoir-free preparation per block, serial scan per stream
constexpr int kChainMaxLinesPerItem = 2 * 1024;  // coded lines one scan item holds (all its streams together)
constexpr int kChainGroups = 5;    // chained encode: the four joint block shapes + Close()'s non-joint long block
struct ChainGroupDev {               // what chain_phase_b_kernel knows about one block-shape group (device memory)
    int joint, nb, nTot, M, K, nEv, maxN, nScaleBits, nstream, pad_;
    double budgetMono, budgetJointPre, blkswA, blkswB;          // codecThem.py:299-308, 381-396
    const unsigned char* bandOfLine;
    const int* bandN;
    const double* lines;             // [n][nsig][M] unscaled MDCT lines (phase A)
    const double* peak;              // [n][nsig][nb] per-band max |X| of the unscaled lines
    const int* oscale;               // [n][nsig] overall scales
    const int* ms;                   // [n][nb] M/S switch (joint groups)
    const unsigned* ev;              // [n][nEv] grant events in np.argmax's order: band | bitsAfter << 6 | nLines << 11
    const unsigned* pre;             // [n][nEv + 1] bits spent before each event if all before it are granted
    int* bitAlloc;                   // [n][nstream][nb]
    int* scaleFactor;                // [n][nstream][nb]
    unsigned short* mant;            // [n][nstream][M]
    int* table;                      // [n][nstream] Huffman table id (15 = raw)
};
size_t chain_events_per_block(const DevShape& S, int joint);
hipError_t launch_chain_prep(const DevShape& S, int joint, int64_t nBlocks, const double* smr, const int* msSwitch,
                             unsigned* ev, unsigned* pre, int forceFallback, hipStream_t st);
// one workgroup per (stream, rate): rate r reads groups[r * kChainGroups ...] and reservoir[r * nStreams + s] and writes its
// trace at resTrace + r * traceStride; the items and phase-A data are shared by all rates
hipError_t launch_chain_phase_b(int64_t nStreams, int nRates, const ChainGroupDev* groups, const int* items,
                                const long long* itemStart, int* reservoir, int* resTrace, long long traceStride,
                                int useHuffman, int threads /* 0: chosen by workgroup count */, hipStream_t st);
hipError_t launch_chain_flush_gather(int64_t nStreams, int L, const void* pcmL, const void* pcmR /* null: mono */, int fmt, int64_t stride,
                                     const long long* tailOffset, void* out, hipStream_t st);
hipError_t launch_chain_headers(int64_t nStreams, int hdrLen, const unsigned char* hdr, const long long* firstChunk,
                                const long long* pos, unsigned char* out, long long outCap, long long* streamPos,
                                hipStream_t st);
// mrc_kernels_target.hip -- the NMR of every rung of a chained ladder from the scan's planes (mrc_encode_chained_target_nmr_pac)
// One workgroup per entry (block k0 + kb, output channel) of n blocks of group g: groups [nRates][kChainGroups] in device
// memory, chunkMap [n * (joint ? 2 : 1)] the entry's chunk in file order, lines / thresh [(joint ? 2 : 1) * n][halfN] the
// source analysis (a joint group: the left rows, then the right rows).  stat[2 * (r * statStride + chunkBase + chunk)] =
// {max_j r_j, b * mean_j r_j} of rung r: launch_nmr_file's input.
hipError_t launch_nmr_rungs(const DevShape& S, int nRates, int joint, int64_t n, int64_t k0, const ChainGroupDev* groups,
                            int g, const long long* chunkMap, const double* lines, const double* thresh, double* stat,
                            long long statStride, long long chunkBase, hipStream_t st);
// span [nStreams][3] = {first byte in `in`, first byte in `out`, length}: byte copies, longest run maxLen
hipError_t launch_target_gather(int64_t nStreams, int64_t maxLen, const long long* span, const unsigned char* in,
                                unsigned char* out, hipStream_t st);
// mrc_kernels_vbr.hip -- constant-quality VBR (mrc_encode_vbr_nmr_pac): per band the fewest bits with noise / mask <= ceiling
// One workgroup per block k0 + kb of n blocks of a group: phaseLines [blocks][joint ? 4 : 1][halfN], oscale, msSwitch are
// phase A's (indexed by the group's block), lines / thresh / chunkMap the source analysis and file order of THIS launch's
// blocks as launch_nmr_rungs takes them.  Writes the group's planes bitAlloc / scaleFactor [blocks][streams][nBands] and mant
// [blocks][streams][halfN], stat[2 * (chunkBase + chunk)] = {max_j r_j, b * mean_j r_j} and capped[chunkBase + chunk] (a
// block's capped bands at its first chunk, 0 at its second).
hipError_t launch_vbr_alloc(const DevShape& S, int joint, int64_t n, int64_t k0, double ceiling, const double* phaseLines,
                            const int* oscale, const int* msSwitch, int* bitAlloc, int* scaleFactor, unsigned short* mant,
                            const long long* chunkMap, const double* lines, const double* thresh, double* stat, int* capped,
                            long long chunkBase, hipStream_t st);
// Encode to a size at constant quality (mrc_encode_vbr_size_pac).  launch_vbr_profile: launch_vbr_alloc's inputs without a
// ceiling; every band walks to the end of its state sequence and its ratios go to prof [blocks of the group][nBands]
// [vbr_profile_bytes / nBands / 8], the streams its M/S bands raised to profPick [blocks of the group][nBands] (joint only).
// launch_vbr_pick: all n blocks of a group at the ceiling of their stream (ceilings [streams], chunkStream [chunks]) from that
// record and phase A's data alone; it writes what launch_vbr_alloc writes (chunkBase 0).  launch_vbr_size_bytes: bytes[s] =
// hdrLen + sum over stream s's chunks of (4 + chunkBytes), the packer's plan in chunk order.
size_t vbr_profile_bytes(const DevShape& S, int joint);   // of one block
size_t vbr_lds_bytes(const DevShape& S, int joint);       // launch_vbr_alloc / _profile refuse more than 60 KB
hipError_t launch_vbr_profile(const DevShape& S, int joint, int64_t n, int64_t k0, const double* phaseLines, const int* oscale,
                              const int* msSwitch, const double* lines, const double* thresh, double* prof, unsigned* profPick,
                              hipStream_t st);
hipError_t launch_vbr_pick(const DevShape& S, int joint, int64_t n, const double* ceilings, const int* chunkStream,
                           const double* phaseLines, const int* oscale, const int* msSwitch, const double* prof,
                           const unsigned* profPick, int* bitAlloc, int* scaleFactor, unsigned short* mant,
                           const long long* chunkMap, double* stat, int* capped, hipStream_t st);
hipError_t launch_vbr_size_bytes(int64_t nStreams, int64_t nChunks, int hdrLen, const long long* firstChunk,
                                 const int* chunkBytes, long long* bytes, hipStream_t st);
// mrc_kernels_huff.hip
hipError_t launch_huffman_gain(const DevShape& S, int64_t nFrames, int nStreams, const int* bitAlloc,
                               const int* mantissa, const int* reservoirOut, int* huffTable, int* bitsSaved,
                               int* reservoirNext, hipStream_t st);
hipError_t launch_bitalloc_cases(int64_t nCases, int nBands, int maxMantBits, const int* nLines,
                                 const double* budget, const double* smr, int* bits, int* left,
                                 double* smrAfter /* nullable: running SMRs after the loop */, hipStream_t st);
hipError_t launch_scale_factor(int64_t n, int nScaleBits, const double* v, const int* nMantBits, int* out,
                               hipStream_t st);
hipError_t launch_mantissa(int64_t n, int nScaleBits, const double* x, const int* scale, const int* nMantBits,
                           int* out, hipStream_t st);
hipError_t launch_transient_peaks(int64_t nHops, int nCh, int hop, int nShort, int nSec, const double* sos, bool unitB0,
                                  const void* streams, int fmt, int64_t chStride, double* peaks, hipStream_t st);
hipError_t launch_stereo_masking(int64_t n, const double* mid, const double* side, const double* z, double* outMid,
                                 double* outSide, hipStream_t st);
hipError_t launch_ms_switch(int64_t nBlocks, int nBands, int nLeaves, int nInternal, const int* plan /* device */,
                            const double* L, const double* R, int64_t blockStride /* doubles between blocks */,
                            int nLines /* lines per block */, int* out, hipStream_t st);

}  // namespace mrc
