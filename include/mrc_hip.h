/*
 * mrc_hip.h -- C ABI of libmrc_hip.so: the MI355X (gfx950) implementation of the per-block ENCODE
 * hot path of laser55/mrcAudioCodec (KBD/transition window -> MDCT -> FFT psychoacoustic masked
 * threshold / SMR -> greedy bit allocation -> scale-factor / mantissa quantise -> per-band M/S).
 *
 * The reference has no FFI of its own: its plugin seam is the Python module `codecThem`
 * (pacfileThem.py:108 `import codecThem as codec`; calls at pacfileThem.py:649 -> 987-994 and
 * 820 -> 996-1003).  The entry points below are what a binding for that seam needs; the drop-in
 * Python module mrcaudiocodec_amd/codecThem.py binds them with ctypes.
 *
 * Conventions: every function returns 0 on success, a negative mrc_status on error
 * (mrc_last_error(h) gives the text); no exceptions cross the ABI; a handle is bound to one HIP
 * device and calls on one handle must be serialised by the caller.  There is NO CPU fallback: if
 * no gfx950 device is usable, mrc_create fails with MRC_ERR_NO_DEVICE.
 * "host" functions take host pointers (C-contiguous, caller-allocated outputs) and copy for the
 * caller; "dev" functions take device pointers (HIP allocations of the handle's device) and enqueue
 * on the given hipStream_t (passed as void*; NULL = the handle's own stream) without synchronising.
 *
 * Block shapes.  A block is `a` samples carried over from the previous call followed by `b` new
 * samples (pacfileThem.py:628-631), N = a+b, N/2 MDCT lines.  With nMDCTLines = 1024 and
 * nSamplesShort = 128 the shapes are (1024,1024) long / 25 bands, (128,128) short / 9 bands and the
 * two transitions (1024,128), (128,1024) with 576 lines / 9 bands (pacfileThem.py:637-645,1192-1210).
 *
 * Dense output layout (per block): overall_scale[nsig], scale_factor[nstream][nBands],
 * bit_alloc[nstream][nBands], mantissa[nstream][N/2] (0 where the band got no bits; the reference
 * omits those bands, codecThem.py:336-350 -- the Python wrapper compacts), reservoir_out.
 * mono: nsig = nstream = 1.  joint stereo: nsig = 4 in the order L,R,M,S (codecThem.py:456-460),
 * nstream = 2 (stream 0 = Mid-or-Left per band, stream 1 = Side-or-Right, codecThem.py:524-551),
 * plus ms_switch[nBands].
 */
#ifndef MRC_HIP_H
#define MRC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRC_VERSION 300            /* 0.3.0 */
#define MRC_MAX_BANDS 32
/* how a channel's samples are held: float64 signed fractions (what pcmfile.py:98 hands the codec) or the file's
 * int16 PCM codes (converted on load, pcmfile.py:91-100); how the mantissa plane is stored */
#define MRC_SAMPLES_F64 0
#define MRC_SAMPLES_PCM16 1
#define MRC_MANTISSA_I32 0
#define MRC_MANTISSA_I16 1         /* uint16: a code is sign bit + magnitude in at most 16 bits (codecThem.py:292-293) */

typedef enum mrc_status {
    MRC_OK = 0,
    MRC_ERR_INVALID = -1,          /* bad argument (shape, sizes, null pointer) */
    MRC_ERR_NO_DEVICE = -2,        /* no usable HIP device / not gfx950 */
    MRC_ERR_HIP = -3,              /* a HIP runtime call failed */
    MRC_ERR_NOMEM = -4
} mrc_status;

/* The codec parameters the path reads from the reference's CodingParams bag
 * (audiofile.py:51-53; values set at pacfileThem.py:1105-1121). */
typedef struct mrc_config {
    int32_t sample_rate;           /* codingParams.sampleRate (integer Hz: py2 `sampleRate/N` is an int division) */
    int32_t n_mdct_lines;          /* codingParams.nMDCTLines, 1024 */
    int32_t n_short;               /* codingParams.nSamplesShort, 128 */
    int32_t n_scale_bits;          /* codingParams.nScaleBits, 4 */
    int32_t n_mant_size_bits;      /* codingParams.nMantSizeBits, 4 */
    int32_t blksw_bits_a;          /* codingParams.blkswBitA, 1 */
    int32_t blksw_bits_b;          /* codingParams.blkswBitB, 1 */
    int32_t device_id;             /* HIP device ordinal */
    double  target_bits_per_sample;/* codingParams.targetBitsPerSample, 2.86 */
} mrc_config;

typedef struct mrc_handle mrc_handle;

int  mrc_version(void);
int  mrc_device_count(void);                              /* number of HIP devices, 0 if none */
void mrc_default_config(mrc_config* cfg);                 /* pacfileThem.py:1105-1121 defaults, 48 kHz, device 0 */
int  mrc_create(const mrc_config* cfg, mrc_handle** out);
void mrc_destroy(mrc_handle* h);
const char* mrc_last_error(const mrc_handle* h);          /* h may be NULL: error of the last failed call without a
                                                            * handle (mrc_create, mrc_band_table, mrc_pac_header,
                                                            * mrc_pac_read_header) */

/* Shape queries (band tables of psychoac.py:86-131 / pacfileThem.py:637-645). */
int  mrc_shape_bands(mrc_handle* h, int a, int b, int32_t* n_bands, int32_t* n_lines /*[MRC_MAX_BANDS]*/);
int  mrc_shape_budget(mrc_handle* h, int a, int b, int joint, int32_t reservoir, double* bit_budget);

/* ---- host entry points: what codecThem.EncodeSingleChannel / JointEncodeChannels bind ---------- */

/* codecThem.py:281-354 for n_blocks independent blocks of one shape.  blocks: [n_blocks][a+b].
 * reservoir_in may be NULL (zeros).  mdct_out (unscaled lines, [n_blocks][N/2]) may be NULL. */
int mrc_encode_mono(mrc_handle* h, int64_t n_blocks, int a, int b, const double* blocks,
                    const int32_t* reservoir_in,
                    int32_t* overall_scale, int32_t* scale_factor, int32_t* bit_alloc,
                    int32_t* mantissa, int32_t* reservoir_out, double* mdct_out);

/* codecThem.py:359-574.  left/right: [n_blocks][a+b].  overall_scale: [n_blocks][4] (L,R,M,S);
 * ms_switch: [n_blocks][nBands]; scale_factor/bit_alloc: [n_blocks][2][nBands];
 * mantissa: [n_blocks][2][N/2]; mdct_out: [n_blocks][4][N/2] or NULL. */
int mrc_encode_joint(mrc_handle* h, int64_t n_blocks, int a, int b, const double* left, const double* right,
                     const int32_t* reservoir_in,
                     int32_t* overall_scale, int32_t* ms_switch, int32_t* scale_factor, int32_t* bit_alloc,
                     int32_t* mantissa, int32_t* reservoir_out, double* mdct_out);

/* The same for n_blocks blocks of MIXED shapes in one call -- a block-switched stream as pacfileThem.py:1192-1210
 * produces it -- so that a binding without array libraries can hand over a whole stream: `blocks` (left / right) is
 * the blocks packed back to back, block i holding a[i] + b[i] samples; SURVEY.md 8(b) `a[]`, `b[]`.  Blocks are grouped
 * by shape inside (one launch set per distinct shape); reservoir_in [n] may be NULL.  Because the shape varies, the
 * outputs have fixed strides: scale_factor / bit_alloc [n][streams][MRC_MAX_BANDS], ms_switch [n][MRC_MAX_BANDS],
 * mantissa [n][streams][n_mdct_lines] dense (entries beyond a block's band / line count are 0), overall_scale
 * [n] (mono) / [n][4] (joint). */
int mrc_encode_mono_blocks(mrc_handle* h, int64_t n_blocks, const double* blocks, const int32_t* a, const int32_t* b,
                           const int32_t* reservoir_in, int32_t* overall_scale, int32_t* scale_factor,
                           int32_t* bit_alloc, int32_t* mantissa, int32_t* reservoir_out);
int mrc_encode_joint_blocks(mrc_handle* h, int64_t n_blocks, const double* left, const double* right, const int32_t* a,
                            const int32_t* b, const int32_t* reservoir_in, int32_t* overall_scale, int32_t* ms_switch,
                            int32_t* scale_factor, int32_t* bit_alloc, int32_t* mantissa, int32_t* reservoir_out);

/* ---- the file's own sample format in, compact codes out: what a WAV -> .pac pipeline moves over PCIe ----------
 * A long-block stream from 16-bit PCM codes in HOST memory to codes in HOST memory, pipelined: pcm_left (and
 * pcm_right: joint stereo) hold (n_frames + 1) * n_mdct_lines int16 samples, hop-overlapped (frame f = samples
 * [f * L, f * L + 2 L); the first hop is the prior block, zeros at file start: pacfileThem.py:615-631).  The codes
 * are converted on load exactly as pcmfile.py:91-100 does (x = 2c/65535 correctly rounded, -32768 -> 0.0).
 * Frames are independent given reservoir_in [n] (NULL = zeros).  Outputs as mrc_encode_mono / _joint for a = b = L,
 * except the mantissa plane, which is uint16 [n][streams][L] (codes are at most 16 bits wide, codecThem.py:292-293).
 * The work is cut into chunks of chunk_frames frames (0: 32 768, fewer for streams shorter than six chunks) over a
 * ring of four chunk buffers; ALL uploads are queued on one HIP stream, all kernels on the handle's stream, all
 * downloads on a third, ordered by events, so chunk i+1 is copied in and chunk i-1 copied out beside chunk i's
 * kernels (one stream per direction: what the copy engines of the MI355X box run fastest).  With host buffers from
 * mrc_host_alloc / mrc_host_register (page-locked) the copies are truly asynchronous; pageable buffers work, slower.
 * PCIe bytes per (frame, channel): 2 048 in, 2 048 + 2 * 4 * nBands + 8 (+ 4 * nBands per joint frame) out. */
int mrc_encode_stream_pcm16(mrc_handle* h, int64_t n_frames, const int16_t* pcm_left, const int16_t* pcm_right,
                            const int32_t* reservoir_in, int32_t* overall_scale, int32_t* ms_switch,
                            int32_t* scale_factor, int32_t* bit_alloc, uint16_t* mantissa16, int32_t* reservoir_out,
                            int64_t chunk_frames);
/* The same pipeline with the back end on the device too (mrc_dev_pack_blocks behind the kernels of every chunk):
 * 16-bit PCM in host memory -> the `.pac` CHUNK BYTES of the frames in host memory, what WriteDataBlock (mono:
 * one chunk per frame) / JointWriteDataBlock (stereo: two) would append frame after frame (pacfileThem.py:652-781,
 * 825-963) -- a WAV -> .pac pipeline is then: this call, file header (mrc_pac_header), write.  Only ~350 bytes per
 * frame and channel come back over PCIe instead of the 2 KB mantissa plane.  Frames independent given
 * reservoir_in [n] (NULL = zeros); use_huffman: price the four tables per chunk (codecThem.py:136-203), else raw.
 * out [out_cap] (size it with n * channels * mrc_pack_bound(cfg, L, L, 1, joint), or less and retry on
 * MRC_ERR_NOMEM), block_offset [n + 1] byte offset of every frame's chunks, total_bytes: the sum; huff_table /
 * bits_saved [n][channels] and reservoir_out [n] may be NULL.  All pointers HOST memory, page-locked for speed. */
int mrc_encode_stream_pcm16_pac(mrc_handle* h, int64_t n_frames, const int16_t* pcm_left, const int16_t* pcm_right,
                                const int32_t* reservoir_in, int use_huffman, uint8_t* out, int64_t out_cap,
                                int64_t* block_offset, int32_t* huff_table, int32_t* bits_saved, int32_t* reservoir_out,
                                int64_t* total_bytes, int64_t chunk_frames);
/* Page-locked host memory (hipHostMalloc / hipHostRegister): no handle needed, any thread. */
int mrc_host_alloc(void** out, size_t bytes);
int mrc_host_free(void* p);
int mrc_host_register(void* p, size_t bytes);
int mrc_host_unregister(void* p);

/* ---- stage-level host entry points (parity tests against the reference's own modules) ---------- */

/* window.py:104-121 (TransitionWindow; KBDWindow when a == b): out[n_blocks][a+b] = blocks * window. */
int mrc_window(mrc_handle* h, int64_t n_blocks, int a, int b, const double* blocks, double* out);
/* mdct.py:63-76 (+ window.py:104-121 when apply_window != 0) + codecThem.py:321-322: MDCT lines
 * (unscaled, [n_blocks][N/2]) and overall scale of each block. */
int mrc_mdct(mrc_handle* h, int64_t n_blocks, int a, int b, const double* blocks, int apply_window,
             double* lines, int32_t* overall_scale);
/* psychoac.py:176-219 (CalcSMRs): smr[n_blocks][nBands]; thresh (masked threshold,
 * psychoac.py:134-173, [n_blocks][N/2]) may be NULL.  scaled_lines [n_blocks][N/2] are the MDCT lines
 * already multiplied by 2^overall_scale[i] as CalcSMRs receives them; pass scaled_lines = NULL (and
 * overall_scale = NULL) to have them computed from `blocks` by the windowed MDCT. */
int mrc_smr(mrc_handle* h, int64_t n_blocks, int a, int b, const double* blocks,
            const double* scaled_lines, const int32_t* overall_scale, double* smr, double* thresh);
/* bitalloc.py:106-155 for n_cases independent problems of n_bands (<= 64) bands each:
 * smr [n_cases][n_bands] (not modified), n_lines [n_bands], budget [n_cases].
 * bits [n_cases][n_bands], bits_left [n_cases] (int(bitsLeft), truncated toward zero). */
int mrc_bitalloc(mrc_handle* h, int64_t n_cases, int n_bands, int max_mant_bits, const int32_t* n_lines,
                 const double* budget, const double* smr, int32_t* bits, int32_t* bits_left);
/* The same with bitalloc.py:132-151's SIDE EFFECT: smr [n_cases][n_bands] is overwritten with the running values the
 * loop leaves behind (-12 for a band's first grant, -6 per further bit, -99999999999999999.0 once retired). */
int mrc_bitalloc_inplace(mrc_handle* h, int64_t n_cases, int n_bands, int max_mant_bits, const int32_t* n_lines,
                         const double* budget, double* smr, int32_t* bits, int32_t* bits_left);
/* quantize.py:114-146 elementwise: scale[i] = ScaleFactor(v[i], n_scale_bits, n_mant_bits[i]). */
int mrc_scale_factor(mrc_handle* h, int64_t n, int n_scale_bits, const double* v, const int32_t* n_mant_bits,
                     int32_t* scale);
/* quantize.py:294-322 elementwise: mant[i] = vMantissa([x[i]], scale[i], n_scale_bits, n_mant_bits[i]). */
int mrc_mantissa(mrc_handle* h, int64_t n, int n_scale_bits, const double* x, const int32_t* scale,
                 const int32_t* n_mant_bits, int32_t* mant);
/* quantize.py:61-87 (vQuantizeUniform; QuantizeUniform 12-38 is its scalar form) elementwise: code[i] = sign bit <<
 * (n_bits - 1) + magnitude code of |x[i]|; 1 <= n_bits <= 62. */
int mrc_quantize_uniform(mrc_handle* h, int64_t n, int n_bits, const double* x, int64_t* code);
/* psychoac.py:27-29 elementwise: z = 13 atan(0.76 f / 1000) + 3.5 atan((f / 7500)^2). */
int mrc_bark(mrc_handle* h, int64_t n, const double* f, double* z);
/* pcmfile.py:91-100 elementwise: out[i] = sign(c) 2|c| / 65535 (one rounding), -32768 -> 0.0 -- the map the PCM16
 * ingest paths apply on load. */
int mrc_pcm_to_float(mrc_handle* h, int64_t n, const int16_t* pcm, double* out);
/* pacfileThem.py:1025-1056 (TransientDetector), numeric part, for every hop of a stream at once: streams is
 * [n_channels][(n_hops+1)*nMDCTLines] (each channel starts with the prior hop); hop i = samples
 * [(i+1)*nMDCTLines, (i+2)*nMDCTLines) is filtered FROM A ZERO STATE (the reference calls sosfilt without zi)
 * by the n_sections second-order sections sos[n_sections][6] = {b0,b1,b2,a0=1,a1,a2} (scipy layout; the
 * reference designs them with signal.cheby2(20,40,9000/fs,'high') + tf2sos, pacfileThem.py:1146-1147).
 * peaks [n_hops][n_channels][nMDCTLines/nSamplesShort + 1]: max |y| of each short sub-block, then of the hop.
 * The threshold tests and the block-shape sequencing (pacfileThem.py:1046-1056, 1182-1214) are host logic:
 * mrcaudiocodec_amd/transient.py. */
int mrc_transient_peaks(mrc_handle* h, int64_t n_hops, int n_channels, int n_sections, const double* sos,
                        const double* streams, double* peaks);
/* ... with the streams given as MRC_SAMPLES_F64 (double*) or MRC_SAMPLES_PCM16 (int16_t*: the WAV's own codes, converted
 * on load as pcmfile.py:91-100 does) */
int mrc_transient_peaks_ex(mrc_handle* h, int64_t n_hops, int n_channels, int n_sections, const double* sos,
                           const void* streams, int sample_format, double* peaks);
/* The same on streams that are already in DEVICE memory, as float64 signed fractions or as the file's int16 PCM codes
 * (converted on load, pcmfile.py:91-100): channel c starts at streams + c * channel_stride samples; peaks (device)
 * [n_hops][n_channels][nMDCTLines/nSamplesShort + 1]; sos is a HOST pointer.  Enqueued on `stream`.  The filter
 * coefficients are staged in a buffer the HANDLE owns: one stream per handle at a time -- a second call on another stream
 * while the first may still run would overwrite (or, growing, free) what its kernel reads; use one handle per stream. */
int mrc_dev_transient_peaks(mrc_handle* h, int64_t n_hops, int n_channels, int n_sections, const double* sos,
                            const void* streams, int sample_format, int64_t channel_stride, double* peaks, void* stream);
/* ms_stereo.py:53-67 elementwise over n lines: out_mid = max(mid, min(side, MLD side)), out_side likewise, MLD from z
 * (Bark).  Kept for the drop-in module's symbol; the encoder's own use of it is dead (psychoac.py:205-210). */
int mrc_stereo_masking_factor(mrc_handle* h, int64_t n, const double* mid_thresh, const double* side_thresh,
                              const double* z, double* out_mid, double* out_side);
/* ms_stereo.py:5-27 for n_blocks pairs of line vectors [n_blocks][n_total_lines] and one band table. */
int mrc_ms_switch(mrc_handle* h, int64_t n_blocks, int n_bands, const int32_t* n_lines,
                  const double* lines_left, const double* lines_right, int32_t* ms_switch);

/* ---- device entry points (batch / stream mode; bench.py and multi-GPU sharding drive mrc_dev_encode_ex) ---- */

/* Frame f of the batch reads its a+b samples at ch[offsets ? offsets[f] : f*frame_stride ...].
 * frame_stride = b  -> an overlapped PCM stream, every hop read once (pacfileThem.py:628-631);
 * frame_stride = a+b -> explicit blocks.  ch_right == NULL -> mono (nsig = 1), else joint (nsig = 4).
 * Buffers (device): lines [n][nsig][N/2] f64, overall_scale [n][nsig] i32, smr [n][nsig][nBands] f64,
 * ms_switch [n][nBands] i32 (joint only), bit_alloc/scale_factor [n][nstream][nBands] i32,
 * mantissa [n][nstream][N/2] i32, reservoir_in (may be NULL) / reservoir_out [n] i32.
 * The three stage calls (mrc_dev_mdct, mrc_dev_smr, mrc_dev_alloc_quant) are neither timed (mrc_set_timing) nor counted
 * by MRC_OPT_SENSITIVITY; mrc_dev_smr computes the SMRs of all nsig signals in every band.  mrc_dev_alloc_quant keeps
 * per-band peaks in the handle's workspace: one stream per handle at a time. */
int mrc_dev_mdct(mrc_handle* h, int a, int b, int64_t n_frames, const double* ch_left, const double* ch_right,
                 int64_t frame_stride, const int64_t* offsets, double* lines, int32_t* overall_scale, void* stream);
int mrc_dev_smr(mrc_handle* h, int a, int b, int64_t n_frames, const double* ch_left, const double* ch_right,
                int64_t frame_stride, const int64_t* offsets, const double* lines, const int32_t* overall_scale,
                double* smr, double* thresh /*nullable*/, void* stream);
/* Everything of the encode that does not depend on the bit reservoir, as the encode calls launch it (the same kernel
 * instantiations, MRC_OPT_SENSITIVITY counted), with the masking kernel's own outputs handed out: smr and band_peak
 * [n][nsig][nBands] f64 (band_peak: max |line| of the band, unscaled).  Joint frames get the SMRs and peaks of the signals
 * the M/S switch selects per band; units that no band selects stay unwritten.  ms_switch: joint only. */
int mrc_dev_masking(mrc_handle* h, int a, int b, int64_t n_frames, const void* ch_left, const void* ch_right,
                    int sample_format, int64_t frame_stride, const int64_t* offsets, double* lines, int32_t* overall_scale,
                    int32_t* ms_switch, double* smr, double* band_peak, void* stream);
/* One __device__ helper of the kernels (cross-lane primitives, 2^x, 1/x, atan, SPL conversion, quantiser templates), called
 * unchanged by a small kernel of its own on the caller's inputs: how the tests hold each helper to its documented bound
 * (tests/test_gpu_helper_probes.py).  All arrays are DEVICE arrays of 8-byte words, word k of element j at [k * n + j]: doubles
 * as their bits, signed integers as int64, unsigned 32-bit values zero-extended.  Words per element of in0, in1, in2 -> out:
 *   MOVES_I32 / _U32 / _F64  a | b -> dpp_move 0xB1, 0x4E, 0x141, 0x128 of a; x, y of rows_swap<16>(a, b); x, y of rows_swap<32>
 *   SUM_F64       1 -> wave_sum, row_reduce(+)          MAX_F64  1 -> wave_max          ROW_MAX  1 -> row_max
 *   REDUCE_I32    1 -> wave_sum_i, wave_max_i, row_reduce(+), row_reduce(max)
 *   FOLD4_F64     4 -> wave_fold4(fmax)                 FOLD4_U32  4 -> wave_fold4(+)
 *   FOLD2         2 (int) | 2 (double) -> wave_fold2(+) of the ints, of the doubles
 *   SUM_BLOCK8    8 -> wave_sum_block<8>                SUM_ALL9 / 16 / 17  N -> wave_sum_all<N>
 *   SCAN_I32 / SCAN_F64  1 -> wave_incl_scan            ORDER_KEY  1 -> order_key, order_value of that key
 *   XCD           b | g -> xcd_contiguous(b, g)         RCP  1 -> the bare hardware reciprocal, recip_nr
 *   LINE_RATIO    a2 | t -> line_ratio                  EXP2_POLY  1 -> exp2_poly
 *   EXP2_TAB      sT | u -> exp2_tab64<64>, <256>, exp2_tab_above<64>, <256>, tables staged in LDS as the masking kernels do
 *   TABLES        none -> element j: entry j mod 64 / 256 of the two staged 2^x tables, kAtanQ[j mod 22], word j mod 128 of the
 *                 staged log10 table
 *   EXP2_DD       hi | lo -> exp2_dd                    DD_ADD  hi, lo | xh, xl -> hi, lo behind dd_add
 *   ATAN_POS      1 -> atan_pos
 *   SPL           x | a2 -> spl_db_tab(x), spl_db(x), log10_tab32(x), excess_plain(x, a2, scale 3) and the threshold it hands out
 *   MAG_CODE      mag | nBits (1..31) -> mag_code<unsigned>, mag_code<long long>
 *   SCALE_MANT    x | scale + (nScaleBits << 8) + (nMantBits << 16)  (1..4, 2..16) -> scale_factor_dev<unsigned>, <long long>,
 *                 mantissa_dev<unsigned>, <long long>
 * threads: the workgroup size, 64, 128 or 256; whole workgroups cover n, a thread past the end computes on element n - 1 and
 * stores nothing.  out_words: the words `out` holds (at least n times the probe's output words).  MRC_ERR_INVALID: an unknown
 * probe, n outside 1 .. 65536, another workgroup size, out too small, a NULL array the probe needs. */
#define MRC_PROBE_MOVES_I32 1
#define MRC_PROBE_MOVES_U32 2
#define MRC_PROBE_MOVES_F64 3
#define MRC_PROBE_SUM_F64 4
#define MRC_PROBE_MAX_F64 5
#define MRC_PROBE_ROW_MAX 6
#define MRC_PROBE_REDUCE_I32 7
#define MRC_PROBE_FOLD4_F64 8
#define MRC_PROBE_FOLD4_U32 9
#define MRC_PROBE_FOLD2 10
#define MRC_PROBE_SUM_BLOCK8 11
#define MRC_PROBE_SUM_ALL9 12
#define MRC_PROBE_SUM_ALL16 13
#define MRC_PROBE_SUM_ALL17 14
#define MRC_PROBE_SCAN_I32 15
#define MRC_PROBE_SCAN_F64 16
#define MRC_PROBE_ORDER_KEY 17
#define MRC_PROBE_XCD 18
#define MRC_PROBE_RCP 19
#define MRC_PROBE_LINE_RATIO 20
#define MRC_PROBE_EXP2_POLY 21
#define MRC_PROBE_EXP2_TAB 22
#define MRC_PROBE_TABLES 23
#define MRC_PROBE_EXP2_DD 24
#define MRC_PROBE_DD_ADD 25
#define MRC_PROBE_ATAN_POS 26
#define MRC_PROBE_SPL 27
#define MRC_PROBE_MAG_CODE 28
#define MRC_PROBE_SCALE_MANT 29
int mrc_dev_helper_probe(mrc_handle* h, int probe, const void* in0, const void* in1, const void* in2, void* out,
                         int64_t out_words, int64_t n, int threads, void* stream);
int mrc_dev_alloc_quant(mrc_handle* h, int a, int b, int64_t n_frames, int joint,
                        const double* lines, const int32_t* overall_scale, const double* smr,
                        const int32_t* reservoir_in, int32_t* ms_switch, int32_t* bit_alloc,
                        int32_t* scale_factor, int32_t* mantissa, int32_t* reservoir_out, void* stream);
/* mrc_dev_alloc_quant through the CHAINED back end (the sorted grant events and the serial scan of the chained encodes, which
 * mrc_encode_mono / mrc_encode_joint also take for 64 blocks or fewer), with the reservoir carried from block to block:
 * consecutive runs of blocks_per_stream (>= 1, dividing n_frames) blocks form a stream; reservoir_in (NULL: zeros) and
 * reservoir_out have one entry per STREAM, reservoir_trace (nullable) [n_frames] the reservoir behind every block.  With
 * use_huffman the cheapest of the four tables is priced per block and channel and its saving goes into the reservoir
 * (codecThem.py:136-180,224,274); huff_table (nullable) [n_frames][nstream] receives the ids (15: raw).  The M/S switch and
 * the band peaks are computed as mrc_dev_alloc_quant computes them.  The mantissa plane is the back end's own:
 * mantissa16 [n][nstream][N/2] uint16 (MRC_MANTISSA_I16), 8-byte aligned; lines 16-byte aligned.  MRC_OPT_CHAIN_THREADS and
 * MRC_OPT_CHAIN_FORCE_REPAIR are honoured.  MRC_ERR_INVALID: a shape outside the chained back end (more than 64 coded bands,
 * more than 2048 coded lines per block, lines not a multiple of 4), a NULL output, a bad blocks_per_stream, a misaligned
 * plane.  Not timed, not counted; workspace in the handle: one stream per handle at a time. */
int mrc_dev_alloc_quant_chained(mrc_handle* h, int a, int b, int64_t n_frames, int joint, int64_t blocks_per_stream,
                                int use_huffman, const double* lines, const int32_t* overall_scale, const double* smr,
                                const int32_t* reservoir_in, int32_t* ms_switch, int32_t* bit_alloc, int32_t* scale_factor,
                                uint16_t* mantissa16, int32_t* huff_table, int32_t* reservoir_out, int32_t* reservoir_trace,
                                void* stream);
/* The three kernels of the constant-quality VBR calls (mrc_encode_vbr_nmr_pac, mrc_encode_vbr_size_pac) on the caller's
 * planes: n_frames independent blocks of shape (a, b), all mono or all joint, through exactly the launches those calls make
 * (first block 0, chunks in block order, every block a stream of its own).  All pointers are device memory.
 *   inputs   lines [n][nsig][N/2] f64 phase A's UNSCALED lines (joint: L, R, M, S); overall_scale [n][nsig] i32;
 *            ms_switch [n][nBands] i32 (joint only, else nullable); source_lines / source_thresh [nstream][n][N/2] f64: the
 *            source analysis X and T (dB) per output channel -- all left rows, then all right rows; ceiling: LINEAR (the
 *            calls' pow(10, dB / 10)), +inf and 0 allowed.
 *   outputs  bit_alloc / scale_factor [n][nstream][nBands] i32; mantissa16 [n][nstream][N/2] uint16; stat [n][nstream][2]
 *            f64 = {max_j r_j, b * mean_j r_j} of the output channel; capped [n][nstream] i32: the block's capped bands at
 *            its first entry, 0 at its second.
 * mrc_dev_vbr_profile hands out the record of the walk without a ceiling: ratios [n][nBands][W] f64, W =
 * mrc_vbr_record_width(joint), first filled with NaN by the entry so that the states the walk wrote can be told; picks
 * [n][nBands] u32 (joint only, else nullable).  Mono band: r at state i (0, 2, 3, .. bits) in [i].  Joint L/R band: stream
 * s's in [s * W / 2 + i].  M/S band: {r_L, r_R} of step i in [2 i], [2 i + 1], bit i of the pick word the stream raised
 * behind step i.  mrc_dev_vbr_pick takes such a record and ceilings [n] f64 (one per block) and leaves what
 * mrc_dev_vbr_alloc leaves at that ceiling.  The planes need their types' natural alignment only.
 * MRC_ERR_INVALID (with a message naming the argument): a NULL plane; a NaN ceiling; n_frames < 0; a shape the handle does
 * not have, one outside the chained back end (more than 2048 coded lines per block, lines not a multiple of 4) or one whose
 * walk the kernels cannot hold (more than MRC_MAX_BANDS bands, more than 60 KB of LDS).  n_frames == 0 returns MRC_OK and
 * writes nothing.  Not timed, not counted; workspace in the handle: one stream per handle
 * at a time. */
int mrc_vbr_record_width(int joint);
int mrc_dev_vbr_alloc(mrc_handle* h, int a, int b, int64_t n_frames, int joint, double ceiling, const double* lines,
                      const int32_t* overall_scale, const int32_t* ms_switch, const double* source_lines,
                      const double* source_thresh, int32_t* bit_alloc, int32_t* scale_factor, uint16_t* mantissa16,
                      double* stat, int32_t* capped, void* stream);
int mrc_dev_vbr_profile(mrc_handle* h, int a, int b, int64_t n_frames, int joint, const double* lines,
                        const int32_t* overall_scale, const int32_t* ms_switch, const double* source_lines,
                        const double* source_thresh, double* ratios, uint32_t* picks, void* stream);
int mrc_dev_vbr_pick(mrc_handle* h, int a, int b, int64_t n_frames, int joint, const double* ceilings, const double* lines,
                     const int32_t* overall_scale, const int32_t* ms_switch, const double* ratios, const uint32_t* picks,
                     int32_t* bit_alloc, int32_t* scale_factor, uint16_t* mantissa16, double* stat, int32_t* capped,
                     void* stream);
/* The three stages back to back, intermediates in the handle's workspace (grown on demand, never
 * inside a timed loop once warm).  lines_out may be NULL. */
int mrc_dev_encode(mrc_handle* h, int a, int b, int64_t n_frames, const double* ch_left, const double* ch_right,
                   int64_t frame_stride, const int64_t* offsets, const int32_t* reservoir_in,
                   int32_t* overall_scale, int32_t* ms_switch, int32_t* bit_alloc, int32_t* scale_factor,
                   int32_t* mantissa, int32_t* reservoir_out, double* lines_out, void* stream);
/* The same with the channel format (MRC_SAMPLES_*: ch_left / ch_right are double* or int16_t*) and the mantissa
 * plane format (MRC_MANTISSA_*: int32_t* or uint16_t*) chosen by the caller; offsets / frame_stride count samples. */
int mrc_dev_encode_ex(mrc_handle* h, int a, int b, int64_t n_frames, const void* ch_left, const void* ch_right,
                      int sample_format, int64_t frame_stride, const int64_t* offsets, const int32_t* reservoir_in,
                      int32_t* overall_scale, int32_t* ms_switch, int32_t* bit_alloc, int32_t* scale_factor,
                      void* mantissa, int mantissa_format, int32_t* reservoir_out, double* lines_out, void* stream);

/* ---- host-side back end: Huffman table choice + `.pac` bit packing (no GPU, no handle) -----------
 * BASELINE.json's north_star keeps huffman.py / bitpack.py on the host; these are their C++ form, fed with
 * the dense outputs of mrc_encode_mono / mrc_encode_joint.  Table ids: sorted names (percussive 0,
 * silence 1, speech 2, tonal 3), 15 = raw mantissas (codecThem.py:149). */

/* psychoac.py:86-105 + pacfileThem.py:637-645: lines per scale-factor band of block shape (a,b).  MRC_ERR_INVALID where the
 * reference's loop raises IndexError: the centre of the shape's last line below 15500 Hz (sample rates below ~31 kHz).
 * mrc_create, mrc_pac_header (all four block shapes of cfg) and mrc_pac_read_header (the long shape) refuse such rates too. */
int mrc_band_table(const mrc_config* cfg, int a, int b, int32_t* n_bands, int32_t* n_lines /*[MRC_MAX_BANDS]*/);
/* Upper bound of the bytes one block can pack to (all its channel chunks, length prefixes included). */
int64_t mrc_pack_bound(const mrc_config* cfg, int a, int b, int n_channels, int joint);
/* pacfileThem.py:586-613 (file header; num_samples is padded by the reference's inverted test). */
int mrc_pac_header(const mrc_config* cfg, int n_channels, uint32_t num_samples, uint8_t* out, int64_t out_cap,
                   int64_t* out_len);
/* Host threads used by mrc_pack_* / mrc_unpack_blocks (process-wide).  Default: the CPUs this process may run on
 * (sched_getaffinity), at most 16, or $MRC_PACK_THREADS. */
int mrc_pack_set_threads(int n_threads);
int mrc_pack_get_threads(void);
/* What PACFile.WriteDataBlock appends per block (pacfileThem.py:652-790) for n_channels independent
 * channels: per channel `<L nBytes` + MSB-first payload {huffTable:4, blkswA, blkswB, overallScale, band
 * records}.  Arrays: overall_scale [n][nch], scale_factor / bit_alloc [n][nch][nBands], mantissa
 * [n][nch][N/2] dense.  use_huffman = 0 writes raw mantissas (EncodeNoHuff), else the table choice of
 * codecThem.py:136-203 runs per channel; huff_table / bits_saved ([n][nch], may be NULL) return the chosen
 * table id and the reservoir credit `bits_saved` (codecThem.py:202,224).  block_offset [n+1] = byte
 * offsets of the blocks in `out`.  Returns MRC_ERR_NOMEM if out_cap is too small. */
int mrc_pack_blocks(const mrc_config* cfg, int64_t n_blocks, int n_channels, int a, int b, int use_huffman,
                    const int32_t* overall_scale, const int32_t* scale_factor, const int32_t* bit_alloc,
                    const int32_t* mantissa, uint8_t* out, int64_t out_cap, int64_t* block_offset,
                    int32_t* huff_table, int32_t* bits_saved);
/* What PACFile.JointWriteDataBlock appends per block (pacfileThem.py:825-970): channel 0 additionally
 * carries overallScale[L,R,M,S] and ms_switch.  overall_scale [n][4], ms_switch [n][nBands], the rest
 * [n][2][...]. */
int mrc_pack_joint_blocks(const mrc_config* cfg, int64_t n_blocks, int a, int b, int use_huffman,
                          const int32_t* overall_scale, const int32_t* ms_switch, const int32_t* scale_factor,
                          const int32_t* bit_alloc, const int32_t* mantissa, uint8_t* out, int64_t out_cap,
                          int64_t* block_offset, int32_t* huff_table, int32_t* bits_saved);

/* The same bytes with the table of every channel chunk GIVEN (huff_table_in [n][nch], ids 0..3 or 15 = raw) -- e.g.
 * the choice mrc_dev_huffman_gain already made on the device -- so the host does not price the four tables again
 * (codecThem.py:151-179); only the recoding and bit packing of codecThem.py:182-200 / pacfileThem.py:716-781,
 * 892-963 remain.  MRC_ERR_INVALID for an id outside {0..3, 15}. */
int mrc_pack_blocks_with_tables(const mrc_config* cfg, int64_t n_blocks, int n_channels, int a, int b,
                                const int32_t* huff_table_in, const int32_t* overall_scale, const int32_t* scale_factor,
                                const int32_t* bit_alloc, const int32_t* mantissa, uint8_t* out, int64_t out_cap,
                                int64_t* block_offset);
int mrc_pack_joint_blocks_with_tables(const mrc_config* cfg, int64_t n_blocks, int a, int b, const int32_t* huff_table_in,
                                      const int32_t* overall_scale, const int32_t* ms_switch,
                                      const int32_t* scale_factor, const int32_t* bit_alloc, const int32_t* mantissa,
                                      uint8_t* out, int64_t out_cap, int64_t* block_offset);

/* The general form of the four packers above: joint = 0 / 1, huff_table_in NULL (price on the host when use_huffman)
 * or given, and the mantissa plane in either format the encoder writes (MRC_MANTISSA_I32: int32_t*, MRC_MANTISSA_I16:
 * uint16_t*, what mrc_encode_stream_pcm16 and mrc_dev_encode_ex deliver) -- no widening copy in between. */
int mrc_pack_blocks_ex(const mrc_config* cfg, int64_t n_blocks, int n_channels, int a, int b, int joint, int use_huffman,
                       const int32_t* huff_table_in, const int32_t* overall_scale, const int32_t* ms_switch,
                       const int32_t* scale_factor, const int32_t* bit_alloc, const void* mantissa, int mantissa_format,
                       uint8_t* out, int64_t out_cap, int64_t* block_offset, int32_t* huff_table, int32_t* bits_saved);

/* Huffman table PRICING on the device (codecThem.py:136-180,202): per (frame, stream) the id of the cheapest
 * table (15 = raw) and bits_saved.  Lets a chained multi-stream encode carry the reservoir from block to block
 * without leaving the GPU; the bytes are produced later by mrc_pack_*.  bit_alloc [n][n_streams][nBands],
 * mantissa [n][n_streams][N/2] dense.  Device form: reservoir_next[f] (may be NULL) = reservoir_out[f] + sum
 * over the frame's streams of bits_saved -- the reservoir the stream's next block starts from (codecThem.py:274). */
int mrc_huffman_gain(mrc_handle* h, int64_t n_blocks, int a, int b, int n_streams, const int32_t* bit_alloc,
                     const int32_t* mantissa, int32_t* huff_table, int32_t* bits_saved);
int mrc_dev_huffman_gain(mrc_handle* h, int a, int b, int64_t n_frames, int n_streams, const int32_t* bit_alloc,
                         const int32_t* mantissa, const int32_t* reservoir_out, int32_t* huff_table,
                         int32_t* bits_saved, int32_t* reservoir_next, void* stream);
/* The `.pac` chunks of n_blocks blocks of ONE shape, packed ON THE DEVICE: the bytes WriteDataBlock /
 * JointWriteDataBlock append per block (pacfileThem.py:652-781, 825-963; bitpack.py:36-101; the Huffman choice
 * and recoding of codecThem.py:136-203) -- byte for byte what mrc_pack_blocks_ex writes on the host, from the
 * encoder's outputs where mrc_dev_encode* left them.  All array arguments are DEVICE pointers, layouts as
 * mrc_pack_blocks_ex: overall_scale [n][joint ? 4 : n_channels], ms_switch [n][nBands] (joint), scale_factor /
 * bit_alloc [n][n_channels][nBands], mantissa [n][n_channels][(a+b)/2] (MRC_MANTISSA_I32 / _I16), huff_table_in
 * [n * n_channels] or NULL (NULL: priced here if use_huffman, else raw).  out [out_cap] receives the chunks
 * (4-byte length + payload each), block_offset [n + 1] the byte offset of every block (last entry: the total);
 * huff_table / bits_saved [n * n_channels] may be NULL.  total_bytes (HOST pointer) non-NULL: the call waits for
 * the stream and returns the total, MRC_ERR_NOMEM if it exceeds out_cap (nothing is written past out_cap; size
 * the buffer with mrc_pack_bound), MRC_ERR_INVALID for a table id outside {0..3, 15} or a chunk beyond mrc_pack_bound
 * (bit_alloc > 16 handed in); NULL: fully asynchronous, read block_offset[n] later -- the packer's workspace belongs to
 * the handle, so asynchronous calls on one handle must all be queued on ONE stream, and errors of an asynchronous
 * call are only seen by mrc_dev_pack_status. */
int mrc_dev_pack_blocks(mrc_handle* h, int a, int b, int64_t n_blocks, int n_channels, int joint, int use_huffman,
                        const int32_t* huff_table_in, const int32_t* overall_scale, const int32_t* ms_switch,
                        const int32_t* scale_factor, const int32_t* bit_alloc, const void* mantissa, int mantissa_format,
                        uint8_t* out, int64_t out_cap, int64_t* block_offset, int32_t* huff_table, int32_t* bits_saved,
                        int64_t* total_bytes, void* stream);
/* Waits for `stream` and returns the status of the most recent mrc_dev_pack_blocks on the handle: MRC_OK,
 * MRC_ERR_INVALID (bad table id / chunk beyond the bound) or MRC_ERR_NOMEM (out_cap exceeded); total_bytes (nullable). */
int mrc_dev_pack_status(mrc_handle* h, int64_t* total_bytes, void* stream);

/* ---- chained stream encode: the reference's WHOLE encode loop in one call ---------------------------------------
 * What `python pacfileThem.py in.wav` does in its encode direction for n_streams stereo streams at once -- one
 * JointWriteDataBlock per block with codingParams.bitReservoir carried from block to block (pacfileThem.py:1159-1214,
 * 793-972; codecThem.py:262-278, 381-396, 503), then Close()'s block through the non-joint writer (973-984), behind the
 * file header (586-613) -- given the block shapes (the transient detector's decisions: mrc_transient_peaks +
 * mrcaudiocodec_amd/transient.py).  The reference runs the whole kernel set once per block because block t+1's bit budget
 * contains what block t left over; here everything that does not depend on the reservoir (window, MDCT, overall
 * scale, SMRs, M/S switch: 95 % of the work) runs as ONE batch per block shape over all blocks of all streams, and the
 * rest (bit allocation -> scale factors -> mantissas -> Huffman pricing -> next reservoir) is a serial scan per stream
 * ON THE DEVICE, one workgroup per stream, no host round trip and no launch per block; the device packer then writes
 * the chunks in file order.
 *   pcm_left / pcm_right [n_streams][stream_stride] int16 PCM codes (converted on load as pcmfile.py:91-100 does); each
 *     stream starts with its prior hop (zeros at file start, pacfileThem.py:615-618).
 *   Blocks of stream s: indices block_start[s] .. block_start[s + 1] - 1 of block_offset / block_a / block_b: block i
 *     reads block_a[i] + block_b[i] samples at block_offset[i] of its stream (the a samples carried over, then the b new
 *     ones, pacfileThem.py:799-802); shapes are the four of the reference's block switching, (L, L), (L, S), (S, S),
 *     (S, L) with L = n_mdct_lines, S = n_short.
 *   reservoir_in [n_streams] (NULL: zeros): codingParams.bitReservoir at the start (pacfileThem.py:1111), e.g. handed
 *     over from the previous shard of a long stream.
 *   use_huffman = 0: EncodeNoHuff's raw mantissas (table id 15).  with_flush: append Close()'s two non-joint chunks
 *     per stream (one for mono streams) (the stream must then end with a long block, as the reference's Close() assumes).
 *   num_samples [n_streams] (NULL: no headers): the header's sample count (the WAV's, pacfileThem.py:1103); the header
 *     of stream s is written in front of its first chunk, so out[stream_byte_offset[s] .. stream_byte_offset[s + 1])
 *     is the complete `.pac` file of stream s.
 *   out [out_cap]: size it with mrc_chain_out_bound, or less and retry on MRC_ERR_NOMEM (total_bytes then holds the
 *     size needed).  item_byte_offset (NULL or [n_items + 1], n_items = blocks + 2 n_streams with_flush): where every
 *     block's chunks start (asked for, the position of every chunk is read back from the device: 8 bytes per chunk; with
 *     NULL only the stream starts come back).  reservoir_out (NULL or [n_streams]): codingParams.bitReservoir after the
 *     last block.
 *     reservoir_trace (NULL or [n_items]): ... after every block (tests).
 * MONO streams: pcm_right == NULL (as in mrc_dev_encode / mrc_encode_stream_pcm16).  The encode loop is then the
 *   reference's with WriteDataBlock in place of JointWriteDataBlock (pacfileThem.py:622-790, codecThem.py:205-231): a
 *   header with nChannels = 1, ONE non-joint chunk per block with the reservoir carried from block to block, and with
 *   with_flush ONE Close() chunk per stream (the last hop followed by a hop of zeros).  n_items = blocks + n_streams
 *   with_flush; item_byte_offset and reservoir_trace hold one entry per item as for stereo.  Everything else -- shapes,
 *   slabs, reservoir_in / reservoir_out, mrc_chain_fetch_output, MRC_OPT_SENSITIVITY -- works as for stereo streams.
 * mrc_dev_encode_chained_pac: the same with pcm_left / pcm_right / out in DEVICE memory (all other pointers host);
 * it synchronises `stream` before it returns (the byte offsets come back).  mrc_get_chain_ms: device time of the last
 * chained call -- ms[0] phase A + preparation, ms[1] the serial scan, ms[2] packing, ms[3] all three.
 * mrc_chain_out_bound: the output bound of a call on stereo streams; mrc_chain_out_bound_ex: of a call on n_channels = 1
 * (mono) or 2 (stereo) streams (mrc_chain_out_bound == mrc_chain_out_bound_ex with 2). */
int64_t mrc_chain_out_bound(mrc_handle* h, int64_t n_streams, const int64_t* block_start, const int32_t* block_a,
                            const int32_t* block_b, int with_flush, int with_headers);
int64_t mrc_chain_out_bound_ex(mrc_handle* h, int n_channels, int64_t n_streams, const int64_t* block_start,
                               const int32_t* block_a, const int32_t* block_b, int with_flush, int with_headers);
int mrc_encode_chained_stream_pcm16_pac(mrc_handle* h, int64_t n_streams, const int16_t* pcm_left, const int16_t* pcm_right,
                                        int64_t stream_stride, const int64_t* block_start, const int64_t* block_offset,
                                        const int32_t* block_a, const int32_t* block_b, const int32_t* reservoir_in,
                                        int use_huffman, int with_flush, const uint32_t* num_samples, uint8_t* out,
                                        int64_t out_cap, int64_t* stream_byte_offset, int64_t* item_byte_offset,
                                        int32_t* reservoir_out, int32_t* reservoir_trace, int64_t* total_bytes);
/* ... with the samples as MRC_SAMPLES_PCM16 (int16_t*) or MRC_SAMPLES_F64 (double*: the signed fractions pcmfile.py:98
 * hands the codec -- what the per-block API takes) */
int mrc_encode_chained_stream_pac(mrc_handle* h, int64_t n_streams, const void* pcm_left, const void* pcm_right,
                                  int sample_format, int64_t stream_stride, const int64_t* block_start,
                                  const int64_t* block_offset, const int32_t* block_a, const int32_t* block_b,
                                  const int32_t* reservoir_in, int use_huffman, int with_flush, const uint32_t* num_samples,
                                  uint8_t* out, int64_t out_cap, int64_t* stream_byte_offset, int64_t* item_byte_offset,
                                  int32_t* reservoir_out, int32_t* reservoir_trace, int64_t* total_bytes);
int mrc_dev_encode_chained_pac(mrc_handle* h, int64_t n_streams, const void* pcm_left, const void* pcm_right,
                               int sample_format, int64_t stream_stride, const int64_t* block_start,
                               const int64_t* block_offset, const int32_t* block_a, const int32_t* block_b,
                               const int32_t* reservoir_in, int use_huffman, int with_flush, const uint32_t* num_samples,
                               uint8_t* out, int64_t out_cap, int64_t* stream_byte_offset, int64_t* item_byte_offset,
                               int32_t* reservoir_out, int32_t* reservoir_trace, int64_t* total_bytes, void* stream);
int mrc_get_chain_ms(mrc_handle* h, double* ms /*[4]*/);

/* ---- rate ladder: one source, several bit rates, one chained call ---------------------------------------------------
 * mrc_encode_chained_ladder_pac encodes the streams of mrc_encode_chained_stream_pac at n_rates target bit rates at once.
 * Output r is byte for byte what mrc_encode_chained_stream_pac writes on a handle whose config is this one's with
 * target_bits_per_sample = target_bits_per_sample[r]: the bytes, the offsets, the reservoirs and the trace, for mono
 * (pcm_right == NULL) and stereo streams, with and without Huffman coding or Close()'s flush, from PCM16 or F64 samples.
 * Nothing the transform, the psychoacoustic model, the M/S switch, the grant-event order or the block shapes compute
 * depends on the rate -- only the bit budget does (codecThem.py:299-306, 381-388) -- so all of that runs ONCE, and the
 * serial scan runs as one workgroup per (rate, stream) side by side, each with its own budgets and reservoir.  The
 * handle's own target_bits_per_sample is ignored and h->cfg is never changed.
 *   n_rates in 1..MRC_MAX_RATES; target_bits_per_sample [n_rates], each finite and in (0, 64].
 *   reservoir_in (NULL: zeros) and reservoir_out (NULL) [n_rates][n_streams]: the reservoir of every (rate, stream).
 *   out [n_rates]: rate r's bytes go to out[r] [out_cap[r]]; size each with mrc_chain_out_bound_ex (the bound does not
 *     depend on the rate).  If any buffer is too small the call returns MRC_ERR_NOMEM with total_bytes[r] filled for EVERY
 *     rate (nothing is written past out_cap[r]); a second call with buffers of those sizes succeeds.
 *   stream_byte_offset [n_rates][n_streams + 1], total_bytes [n_rates]; item_byte_offset (NULL or [n_rates][n_items + 1])
 *     and reservoir_trace (NULL or [n_rates][n_items]) with n_items as for mrc_encode_chained_stream_pac.
 *   MRC_ERR_INVALID, with a message naming the argument, for n_rates outside 1..MRC_MAX_RATES, a rate that is not finite
 *   or outside (0, 64], a NULL out[r], and with MRC_OPT_SENSITIVITY on (the certificate covers one rate).
 * Slabs (MRC_OPT_CHAIN_SLAB_BLOCKS) hold all rates; a ladder's slab takes fewer blocks, so that its device memory stays
 * about that of a one-rate slab.  After a ladder call mrc_chain_fetch_output holds nothing (MRC_ERR_INVALID).
 * mrc_dev_encode_chained_ladder_pac: the same with pcm_left / pcm_right and every out[r] in DEVICE memory (the array
 * `out` itself and all other pointers host); it synchronises `stream` before it returns. */
#define MRC_MAX_RATES 16
int mrc_encode_chained_ladder_pac(mrc_handle* h, int n_rates, const double* target_bits_per_sample /*[n_rates]*/,
                                  int64_t n_streams, const void* pcm_left, const void* pcm_right, int sample_format,
                                  int64_t stream_stride, const int64_t* block_start, const int64_t* block_offset,
                                  const int32_t* block_a, const int32_t* block_b,
                                  const int32_t* reservoir_in /* NULL or [n_rates][n_streams] */, int use_huffman,
                                  int with_flush, const uint32_t* num_samples, uint8_t* const* out /*[n_rates]*/,
                                  const int64_t* out_cap /*[n_rates]*/, int64_t* stream_byte_offset /*[n_rates][n_streams + 1]*/,
                                  int64_t* item_byte_offset /* NULL or [n_rates][n_items + 1] */,
                                  int32_t* reservoir_out /* NULL or [n_rates][n_streams] */,
                                  int32_t* reservoir_trace /* NULL or [n_rates][n_items] */, int64_t* total_bytes /*[n_rates]*/);
int mrc_dev_encode_chained_ladder_pac(mrc_handle* h, int n_rates, const double* target_bits_per_sample, int64_t n_streams,
                                      const void* pcm_left, const void* pcm_right, int sample_format, int64_t stream_stride,
                                      const int64_t* block_start, const int64_t* block_offset, const int32_t* block_a,
                                      const int32_t* block_b, const int32_t* reservoir_in, int use_huffman, int with_flush,
                                      const uint32_t* num_samples, uint8_t* const* out, const int64_t* out_cap,
                                      int64_t* stream_byte_offset, int64_t* item_byte_offset, int32_t* reservoir_out,
                                      int32_t* reservoir_trace, int64_t* total_bytes, void* stream);

/* ---- encode to a target noise-to-mask ratio: one source, a rate ladder, the cheapest rung that is clean enough ---------
 * mrc_encode_chained_target_nmr_pac encodes every stream at the n_rates rates of a ladder (as
 * mrc_encode_chained_ladder_pac does: transform and psychoacoustic model once, the serial scan per (rate, stream)), measures
 * the noise-to-mask ratio of every rung on the device from the scan's own planes while they are resident, and returns per
 * stream the `.pac` file of the LOWEST rung whose nmr_total_db meets the target, with the NMR numbers of every rung.
 * The bytes of the other rungs never leave the device.
 * Whole files only: the call always writes Close()'s flush and the headers (num_samples must not be NULL), the samples are
 * 16-bit PCM (the NMR's source is int16), pcm_right == NULL means mono streams.
 * The rule, per stream s: chosen[s] is the smallest r with nmr_total_db[r][s] <= target_nmr_total_db and met[s] = 1; if no
 * rung meets it, chosen[s] = n_rates - 1 and met[s] = 0.  The comparison is made on the double dB value returned; -inf
 * (silence) meets every target.  out[stream_byte_offset[s] .. stream_byte_offset[s + 1]) is the complete file of stream s
 * at target_bits_per_sample[chosen[s]], byte for byte what mrc_encode_chained_ladder_pac writes for that rung and stream.
 * The numbers: nmr_total_db[r][s], nmr_max_db[r][s], disturbed_blocks[r][s] and n_blocks[s] are the SAME doubles and counts
 * mrc_pac_nmr returns for rung r's file of stream s against the stream's own row from sample n_mdct_lines on, with
 * src_frames = (end of the stream's last block) - n_mdct_lines -- provided the row's first n_mdct_lines samples (the prior
 * hop) are zero.  Every sum is kept in mrc_pac_nmr's order (the same source analysis calls, MRC_OPT_EXACT_SPREAD
 * honoured, the same line decoder, the same band and file reductions), and the results do not depend on what shares the
 * call or on the slab size.
 *   MRC_ERR_INVALID, with a message naming the argument and before any device work, for: n_rates outside
 *   1..MRC_MAX_RATES; a rate that is not finite or outside (0, 64]; rates not strictly ascending; a NaN target (+inf: rung
 *   0, -inf: met only by silence); num_samples == NULL; MRC_OPT_SENSITIVITY on; a stream whose first block has
 *   block_a != n_mdct_lines; a stream where block_offset[i] is not the sum of block_a of its earlier blocks (the NMR
 *   positions blocks by that sum); a stream that does not end in a long block.
 *   out [out_cap]: the bound is mrc_chain_out_bound_ex for ONE rate.  Too small: MRC_ERR_NOMEM with total_bytes and every
 *   result array filled and nothing written past out_cap; the chosen bytes stay on the device for mrc_chain_fetch_output.
 * Slabs (MRC_OPT_CHAIN_SLAB_BLOCKS) apply as for the ladder.  Whole streams of a slab are decided when the slab is done.  For
 * a stream cut into time slabs the per-entry statistics (16 bytes per entry and rung) and the packed bytes of ALL rungs stay
 * on the device until the stream's last slab decides: packed bytes are about 1 % of phase A's footprint per block and
 * rung, so a stream of any length the ladder can encode fits.  The chosen files of the whole call are kept on the device
 * (the sum of the chosen sizes) until the call returns.
 * mrc_dev_encode_chained_target_nmr_pac: pcm_left / pcm_right and out in DEVICE memory, all other pointers host; it
 * synchronises `stream` before it returns.
 * mrc_get_target_ms: device time of the last call, ms: phase A + preparation, the serial scan, the NMR kernels (threshold
 * pass and file reduction included), pack + gather. */
int mrc_encode_chained_target_nmr_pac(mrc_handle* h, int n_rates, const double* target_bits_per_sample /*[n_rates]*/,
                                      double target_nmr_total_db, int64_t n_streams, const int16_t* pcm_left,
                                      const int16_t* pcm_right, int64_t stream_stride, const int64_t* block_start,
                                      const int64_t* block_offset, const int32_t* block_a, const int32_t* block_b,
                                      int use_huffman, const uint32_t* num_samples, uint8_t* out, int64_t out_cap,
                                      int64_t* stream_byte_offset /*[n_streams + 1]*/, int32_t* chosen /*[n_streams]*/,
                                      int32_t* met /*[n_streams]*/, double* nmr_total_db /*[n_rates][n_streams]*/,
                                      double* nmr_max_db /*[n_rates][n_streams]*/,
                                      int64_t* disturbed_blocks /*[n_rates][n_streams]*/, int64_t* n_blocks /*[n_streams]*/,
                                      int64_t* total_bytes);
int mrc_dev_encode_chained_target_nmr_pac(mrc_handle* h, int n_rates, const double* target_bits_per_sample,
                                          double target_nmr_total_db, int64_t n_streams, const int16_t* pcm_left,
                                          const int16_t* pcm_right, int64_t stream_stride, const int64_t* block_start,
                                          const int64_t* block_offset, const int32_t* block_a, const int32_t* block_b,
                                          int use_huffman, const uint32_t* num_samples, uint8_t* out, int64_t out_cap,
                                          int64_t* stream_byte_offset, int32_t* chosen, int32_t* met, double* nmr_total_db,
                                          double* nmr_max_db, int64_t* disturbed_blocks, int64_t* n_blocks,
                                          int64_t* total_bytes, void* stream);
int mrc_get_target_ms(mrc_handle* h, double* ms /*[4]*/);

/* ---- constant-quality VBR: every band coded to a noise-to-mask ceiling -------------------------------------------------
 * mrc_encode_vbr_nmr_pac encodes whole streams without a bit budget and without a reservoir: block shapes, window, MDCT,
 * overall scales, the M/S switch, the quantiser (ScaleFactor, vMantissa) and the file format are the chained call's, but
 * every band of every block gets the FEWEST mantissa bits (0, 2, 3, .., 2^n_mant_size_bits capped at 16, tried in that
 * order) at which its measured noise-to-mask ratio r_j = noise_j / mask_j, as mrc_pac_nmr defines it, is <= the ceiling
 * c = 10^(ceiling_db / 10); c is formed once on the host and returned in *ceiling_ratio.  A band that misses c even at the
 * most bits keeps them and is counted in capped_bands[s].  In a joint block an L/R band is first-fit per coded stream
 * against its own channel; an M/S band starts at (0, 0) and, while max(r_L, r_R) > c, raises the stream (0 -> 2, else + 1)
 * whose own error energy is larger (a tie: stream 0), the other one when that stream is at the most bits; when both are,
 * the band is capped (counted once).  A band without lines takes 0 bits.  DESIGN.md section 12 states the rule in full.
 * The Huffman table of a chunk is calculateHuffmanGain's choice (15 = raw with use_huffman == 0).  A block depends on its
 * own samples only, so one long stream encodes with the parallelism of a batch.
 * Whole files only: headers and Close()'s flush always (num_samples must not be NULL), 16-bit PCM, pcm_right == NULL means
 * mono streams.  out[stream_byte_offset[s] .. stream_byte_offset[s + 1]) is the complete file of stream s.
 * The numbers: nmr_total_db[s], nmr_max_db[s], disturbed_blocks[s] and n_blocks[s] are the SAME doubles and counts
 * mrc_pac_nmr returns for that file against the stream's own row from sample n_mdct_lines on, with src_frames = (end of the
 * stream's last block) - n_mdct_lines, provided the row's first n_mdct_lines samples are zero (every sum in mrc_pac_nmr's
 * order, the same source analysis calls, MRC_OPT_EXACT_SPREAD honoured); where capped_bands[s] == 0, max r <= c holds
 * exactly.  coded_bits[s]: the payload bits of the stream's file, 8 x (its bytes - the file header - 4 per chunk).
 * +inf ceiling: 0 bits everywhere; -inf (c = 0): met only where the noise is exactly 0.  Results do not depend on the
 * slab size (MRC_OPT_CHAIN_SLAB_BLOCKS), on what shares the call, or on its size.
 *   MRC_ERR_INVALID, with a message naming the argument and before any device work, for: a NaN ceiling_db; num_samples ==
 *   NULL; MRC_OPT_SENSITIVITY on; the block layouts mrc_encode_chained_target_nmr_pac refuses (first block_a !=
 *   n_mdct_lines, block_offset[i] not the sum of the stream's earlier block_a, no long block at the end).
 *   out [out_cap]: the bound is mrc_chain_out_bound_ex.  Too small: MRC_ERR_NOMEM with total_bytes and every result array
 *   filled; a call of one slab keeps its bytes on the device for mrc_chain_fetch_output, as mrc_encode_chained_stream_pac does.
 * mrc_dev_encode_vbr_nmr_pac: pcm_left / pcm_right and out in DEVICE memory, all other pointers host; it synchronises
 * `stream` before it returns.
 * mrc_get_vbr_ms: device time of the last call, ms: phase A + source analysis (uploads included), the allocator kernel,
 * pack, the sum of the three (the file reduction, a few microseconds per slab, is outside them). */
int mrc_encode_vbr_nmr_pac(mrc_handle* h, double ceiling_db, int64_t n_streams, const int16_t* pcm_left, const int16_t* pcm_right,
                           int64_t stream_stride, const int64_t* block_start, const int64_t* block_offset,
                           const int32_t* block_a, const int32_t* block_b, int use_huffman, const uint32_t* num_samples,
                           uint8_t* out, int64_t out_cap, int64_t* stream_byte_offset /*[n_streams + 1]*/,
                           double* ceiling_ratio, int64_t* capped_bands /*[n_streams]*/, int64_t* coded_bits /*[n_streams]*/,
                           double* nmr_total_db /*[n_streams]*/, double* nmr_max_db /*[n_streams]*/,
                           int64_t* disturbed_blocks /*[n_streams]*/, int64_t* n_blocks /*[n_streams]*/, int64_t* total_bytes);
int mrc_dev_encode_vbr_nmr_pac(mrc_handle* h, double ceiling_db, int64_t n_streams, const int16_t* pcm_left,
                               const int16_t* pcm_right, int64_t stream_stride, const int64_t* block_start,
                               const int64_t* block_offset, const int32_t* block_a, const int32_t* block_b, int use_huffman,
                               const uint32_t* num_samples, uint8_t* out, int64_t out_cap, int64_t* stream_byte_offset,
                               double* ceiling_ratio, int64_t* capped_bands, int64_t* coded_bits, double* nmr_total_db,
                               double* nmr_max_db, int64_t* disturbed_blocks, int64_t* n_blocks, int64_t* total_bytes,
                               void* stream);
int mrc_get_vbr_ms(mrc_handle* h, double* ms /*[4]*/);

/* ---- constant-quality VBR to a file size ("two-pass VBR") ---------------------------------------------------------------
 * mrc_encode_vbr_size_pac is mrc_encode_vbr_nmr_pac with the ceiling SEARCHED per stream: the best constant quality on a grid
 * of ceilings whose file fits target_bytes[s] (the complete file of stream s: header and the 4-byte length of every chunk
 * included).  Same stream arguments, whole files only, 16-bit PCM, pcm_right == NULL means mono, same outputs.
 *   The grid: db_i = ceiling_lo_db + (double)i * ceiling_step_db (one multiply, one add, in double), i = 0 .. n_ceilings - 1,
 *   c_i = pow(10.0, db_i / 10.0) formed on the host as mrc_encode_vbr_nmr_pac forms its c.  Index 0 is the tightest ceiling.
 *   The rule, per stream s, with bytes(i) the size of the file mrc_encode_vbr_nmr_pac writes for it at ceiling_db = db_i,
 *   lo = 0, hi = n_ceilings - 1:  probe hi;  bytes(hi) > target_bytes[s]: chosen = hi, met = 0, stop;  otherwise met = 1 and
 *   while lo < hi: mid = (lo + hi) / 2, probe mid, bytes(mid) <= target_bytes[s] ? hi = mid : lo = mid + 1;  chosen = hi.
 *   File size is not guaranteed to be monotone in the ceiling, so the contract is this rule, not "the optimum": met == 1
 *   implies the returned file is <= target_bytes[s].
 * out[stream_byte_offset[s] .. stream_byte_offset[s + 1]) is byte for byte the file mrc_encode_vbr_nmr_pac writes for stream
 * s at ceiling_db = chosen_db[s]; capped_bands, coded_bits, nmr_total_db, nmr_max_db, disturbed_blocks and n_blocks are that
 * call's values for that file.  chosen[s]: the grid index, chosen_db[s] = db_chosen, ceiling_ratio[s] = c_chosen, met[s],
 * probes[s]: the ceilings tried (<= MRC_MAX_PROBES).  probe_index / probe_bytes: NULL or [n_streams][MRC_MAX_PROBES], the
 * grid index and file size of every probe in order, -1 in unused entries.  Streams of one call search independently; results
 * do not depend on what shares the call nor on MRC_OPT_CHAIN_SLAB_BLOCKS.  MRC_OPT_EXACT_SPREAD is honoured.
 * How: the sequence of states a band walks through in mrc_encode_vbr_nmr_pac's allocator is fixed by the signal -- c only
 * decides where the walk stops -- so it is recorded once per block (about 12 KB per joint long block, which this call's slabs
 * make room for) and every probe is a lookup, one quantise pass and the packer's pricing: the source analysis and phase A
 * run once per call.  DESIGN.md section 13.
 *   MRC_ERR_INVALID, with a message naming the argument and before any device work, for: all mrc_encode_vbr_nmr_pac refuses;
 *   a non-finite ceiling_lo_db or ceiling_step_db; ceiling_step_db <= 0; n_ceilings outside 1..MRC_MAX_CEILINGS; target_bytes
 *   NULL or an entry negative; a stream with more blocks than a slab of this call holds (it would run in time slabs, and the
 *   search needs all blocks of a stream resident: raise MRC_OPT_CHAIN_SLAB_BLOCKS).
 *   out_cap too small: MRC_ERR_NOMEM as in mrc_encode_vbr_nmr_pac (every result filled, mrc_chain_fetch_output for one slab).
 * mrc_dev_encode_vbr_size_pac: pcm_left / pcm_right and out in DEVICE memory, all other pointers host; it synchronises
 * `stream` before it returns.
 * mrc_get_vbr_size_ms: device time of the last call, ms: phase A + source analysis, the profile kernel, all probes (pick +
 * pricing + size reduction + copy back), the final pick + pack, the sum. */
#define MRC_MAX_CEILINGS 256
#define MRC_MAX_PROBES 9
int mrc_encode_vbr_size_pac(mrc_handle* h, double ceiling_lo_db, double ceiling_step_db, int n_ceilings,
                            const int64_t* target_bytes /*[n_streams]*/, int64_t n_streams, const int16_t* pcm_left,
                            const int16_t* pcm_right, int64_t stream_stride, const int64_t* block_start,
                            const int64_t* block_offset, const int32_t* block_a, const int32_t* block_b, int use_huffman,
                            const uint32_t* num_samples, uint8_t* out, int64_t out_cap,
                            int64_t* stream_byte_offset /*[n_streams + 1]*/, int32_t* chosen /*[n_streams]*/,
                            double* chosen_db /*[n_streams]*/, double* ceiling_ratio /*[n_streams]*/, int32_t* met /*[n_streams]*/,
                            int32_t* probes /*[n_streams]*/, int32_t* probe_index /* NULL or [n_streams][MRC_MAX_PROBES] */,
                            int64_t* probe_bytes /* NULL or [n_streams][MRC_MAX_PROBES] */, int64_t* capped_bands,
                            int64_t* coded_bits, double* nmr_total_db, double* nmr_max_db, int64_t* disturbed_blocks,
                            int64_t* n_blocks, int64_t* total_bytes);
int mrc_dev_encode_vbr_size_pac(mrc_handle* h, double ceiling_lo_db, double ceiling_step_db, int n_ceilings,
                                const int64_t* target_bytes, int64_t n_streams, const int16_t* pcm_left,
                                const int16_t* pcm_right, int64_t stream_stride, const int64_t* block_start,
                                const int64_t* block_offset, const int32_t* block_a, const int32_t* block_b, int use_huffman,
                                const uint32_t* num_samples, uint8_t* out, int64_t out_cap, int64_t* stream_byte_offset,
                                int32_t* chosen, double* chosen_db, double* ceiling_ratio, int32_t* met, int32_t* probes,
                                int32_t* probe_index, int64_t* probe_bytes, int64_t* capped_bands, int64_t* coded_bits,
                                double* nmr_total_db, double* nmr_max_db, int64_t* disturbed_blocks, int64_t* n_blocks,
                                int64_t* total_bytes, void* stream);
int mrc_get_vbr_size_ms(mrc_handle* h, double* ms /*[5]*/);

/* ---- sensitivity certificate (round 4) ----
 * Bit-identity of the integers with the reference is an empirical, counted result: each of them is a floor / compare of
 * float64 values whose last bits differ between implementations (FFT factorisation, log10 / atan / 2^x), and it can only come
 * out differently where the deciding value lies within that difference of its edge.  With MRC_OPT_SENSITIVITY set, the
 * encode calls of a handle count those places; counts [MRC_SENS_COUNT] accumulate until reset:
 *   MRC_SENS_QUANT     mantissa codes within 4e-13 (of the block's scaled peak) of their truncation edge, and scale factors
 *                      decided by a band peak that close to a power-of-two code (quantize.py:12-38,114-146,294-322)
 *   MRC_SENS_BITALLOC  pairs of bands whose SMRs are a multiple of 6 dB apart to within 1e-9 dB: their running values tie
 *                      at some step of the greedy loop (bitalloc.py:132-151, np.argmax)
 *   MRC_SENS_MS        bands whose M/S test is within 1e-12 (relative) of its 0.8 threshold (ms_stereo.py:5-27)
 *   MRC_SENS_PEAK      spectral bins within 1e-11 (relative) of a neighbour they have to beat strictly (psychoac.py:162)
 *   MRC_SENS_NODES     64-line chunks the slope-node evaluation of the masking sum sent back to the sorted sweep (its error
 *                      bound exceeded 1e-13 of a line's masked intensity) -- informational: the result is then the sweep's.
 *                      Mono long blocks evaluate only the lines that can be their band's maximum: there a chunk is sent
 *                      back, and counted, when the bound fails on one of THOSE lines -- or on any line of a chunk that is
 *                      evaluated whole (a line at the SPL floor; a wave with more than 64 such lines)
 *   MRC_SENS_FRAMES    blocks examined
 * A call whose first four counts are zero took no decision near an edge.  Not counted: the overall scale (a 20-bit code of
 * the block peak), the transient detector's threshold tests.  Waits for the whole device (hipDeviceSynchronize), so that
 * counting calls queued on any stream are included; a reset is complete when it returns. */
#define MRC_SENS_QUANT 0
#define MRC_SENS_BITALLOC 1
#define MRC_SENS_MS 2
#define MRC_SENS_PEAK 3
#define MRC_SENS_NODES 4
#define MRC_SENS_FRAMES 5
#define MRC_SENS_COUNT 8
int mrc_get_sensitivity(mrc_handle* h, int64_t* counts /*[MRC_SENS_COUNT]*/, int reset);
/* mrc_chain_fetch_output: the bytes of the LAST mrc_encode_chained_stream[_pcm16]_pac call on this handle, which stay in the
 * handle's device buffer until the next chained call: after MRC_ERR_NOMEM ("out_cap too small") a caller allocates
 * total_bytes and fetches them -- no second encode.  After mrc_encode_chained_target_nmr_pac: the chosen files of that call.  After a rate ladder call nothing is held (MRC_ERR_INVALID).  The offsets / reservoirs of that call were already returned by it. */
int mrc_chain_fetch_output(mrc_handle* h, uint8_t* out, int64_t out_cap, int64_t* total_bytes);

/* ---- decode side ("next" row f-4: the reference's decoder, pacfileThem.py:130-585 + codecThem.py:30-134) ----
 * Host: header and chunk parsing (no GPU, no handle).  Device: dequantise -> undo the overall scale -> M/S
 * reconstruction -> IMDCT -> transition window -> overlap-and-add, and the 16-bit PCM codes. */

/* pacfileThem.py:130-158.  Fills sample_rate, n_mdct_lines, n_scale_bits, n_mant_size_bits of *cfg (other fields
 * untouched); data_offset = first chunk.  The header is untrusted input; accepted is what mrc_pac_header and a handle can
 * write: 1 or 2 channels, a positive rate, 1..4 scale bits, 1..8 allocation-field bits, and 16 <= n_mdct_lines <= 8192 that
 * is even and has no prime factor but 2 and 3 (mrc_create's rule for the long block: N/4 and N/2 factor into 2s and 3s --
 * 1024, 768, 576, 512, 384, ...), for which the rate has a band table.  Anything else: MRC_ERR_INVALID, "header field out of
 * range" (or the band table's own text) in mrc_last_error(NULL). */
int mrc_pac_read_header(const uint8_t* buf, int64_t len, mrc_config* cfg, int32_t* n_channels, uint32_t* num_samples,
                        int64_t* data_offset);
/* Offsets of the `<L nBytes` + payload chunks after the header; returns their number (chunk_offset may be NULL /
 * cap 0 to count), < 0 if a chunk is truncated. */
int64_t mrc_pac_scan_chunks(const uint8_t* buf, int64_t len, int64_t data_offset, int64_t* chunk_offset, int64_t cap);
/* The parsing half of PACFile.ReadDataBlock (pacfileThem.py:176-302, joint = 0) / JointReadDataBlock (341-560,
 * joint = 1, two chunks per block): table id, block-switch bits -> (a, b), overall scale(s), M/S switch, band
 * records with raw or Huffman-coded mantissas (prefix decoding by table; ids in sorted-name order).  Fixed strides
 * because the shape varies from block to block: overall_scale [n][joint ? 4 : n_channels], ms_switch
 * [n][MRC_MAX_BANDS], huff_table [n][n_channels], scale_factor / bit_alloc [n][n_channels][MRC_MAX_BANDS], mantissa
 * [n][n_channels][n_mdct_lines] dense.  chunk_offset [n * n_channels].  A refusal (MRC_ERR_INVALID) names the first chunk
 * refused and why in mrc_last_error(NULL), "mrc_unpack_blocks: chunk at byte <offset>: <reason>", the reason in the words
 * mrc_decode_pac_pcm16, the store and mrc_pac_nmr use for the same chunk. */
int mrc_unpack_blocks(const mrc_config* cfg, int64_t n_blocks, int n_channels, int joint, const uint8_t* buf, int64_t len,
                      const int64_t* chunk_offset, int32_t* a, int32_t* b, int32_t* huff_table, int32_t* overall_scale,
                      int32_t* ms_switch, int32_t* scale_factor, int32_t* bit_alloc, int32_t* mantissa);

/* codecThem.Decode (30-63; n_streams = 1, overall_scale [n]) / JointDecode (65-134; n_streams = 2, overall_scale
 * [n][4] = L,R,M,S, ms_switch [n][nBands]) for n blocks of shape (a, b): scale_factor / bit_alloc [n][n_streams][nBands],
 * mantissa [n][n_streams][N/2] dense -> windowed blocks out [n][n_streams][a+b] (before overlap-and-add). */
int mrc_decode(mrc_handle* h, int64_t n_blocks, int a, int b, int n_streams, const int32_t* overall_scale,
               const int32_t* ms_switch, const int32_t* scale_factor, const int32_t* bit_alloc, const int32_t* mantissa,
               double* out);
/* Device form with the overlap-and-add of pacfileThem.py:312-315 fused: block i ADDS its a+b windowed samples to
 * out_left (and out_right) starting at sample out_offset[i]; the caller zeroes the outputs first.  Every sample
 * receives at most two contributions, so the sum does not depend on the order of the blocks. */
int mrc_dev_decode(mrc_handle* h, int a, int b, int64_t n_blocks, int n_streams, const int32_t* overall_scale,
                   const int32_t* ms_switch, const int32_t* scale_factor, const int32_t* bit_alloc,
                   const int32_t* mantissa, const int64_t* out_offset, double* out_left, double* out_right, void* stream);
/* pcmfile.py:163-172: signed fractions -> 16-bit PCM codes (sign-magnitude quantiser of quantize.py:61-87, then
 * 2's complement).  mrc_pcm16: host pointers; mrc_dev_pcm16: device pointers. */
int mrc_pcm16(mrc_handle* h, int64_t n, const double* x, int16_t* out);
int mrc_dev_pcm16(mrc_handle* h, int64_t n, const double* x, int16_t* out, void* stream);

/* ---- decode on the device (round 5: SURVEY 8 row f-4) ----
 * The chunk parser of mrc_unpack_blocks runs on the device too (csrc/mrc_unpack.hpp, one lane per channel chunk).
 *
 * mrc_dev_unpack_blocks: the same contract and fixed-stride layout as mrc_unpack_blocks (pacfileThem.py:176-302 /
 * 341-560), every array -- buf [len], chunk_offset [n_blocks * n_channels] and the outputs -- in device memory; the
 * codec parameters are the handle's.  Synchronises `stream`; MRC_ERR_INVALID exactly where the host parser refuses:
 * a chunk outside buf, a read past a chunk's end, a table id outside {0..3, 15}, a stored allocation above 16 bits,
 * bits that are no code of the chunk's Huffman table, the chunks of one block in different shapes (mrc_last_error names
 * the first bad chunk).  The outputs are then unspecified. */
int mrc_dev_unpack_blocks(mrc_handle* h, int64_t n_blocks, int n_channels, int joint, const uint8_t* buf, int64_t len,
                          const int64_t* chunk_offset, int32_t* a, int32_t* b, int32_t* huff_table, int32_t* overall_scale,
                          int32_t* ms_switch, int32_t* scale_factor, int32_t* bit_alloc, int32_t* mantissa, void* stream);
/* mrc_decode_pac_pcm16: n_files whole `.pac` files -- file f is buf[file_offset[f], file_offset[f + 1]), host memory,
 * pageable or not -- to 16-bit PCM in host memory, in ONE call: the bytes cross PCIe once, chunk parsing, Huffman
 * decoding, dequantisation, IMDCT, overlap-add (pacfileThem.py:302-315, codecThem.py:30-134) and the codes of
 * pcmfile.py:163-172 run on the device.  File f's samples go to out[sample_offset[f], sample_offset[f + 1]) interleaved
 * in WAV order (pcmfile.py:141-153: sample t of channel c at t * n_channels[f] + c), the first n_mdct_lines samples of
 * each file -- the MDCT's half-block delay -- dropped as the reference's decode loop drops them (pacfileThem.py:1176-1179).
 * Bit-identical to mrc_unpack_blocks + mrc_dev_decode per block shape + mrc_dev_pcm16 (pacfile.decode_pac_pcm16).
 * Every file must carry the handle's sample_rate, n_mdct_lines, n_scale_bits and n_mant_size_bits (else
 * MRC_ERR_INVALID, the text names the file); mono and stereo files may be mixed; a file with a header and no chunks
 * decodes to no samples.  out_cap counts int16 values: if it is too small the call returns MRC_ERR_NOMEM before any
 * device work, writes nothing to out and still fills sample_offset [n_files + 1] (sample_offset[n_files] = the size
 * needed) and n_channels [n_files].  Device memory: the handle's, reused from call to call (~9 bytes per coded line
 * and 16 per output sample and channel). */
int mrc_decode_pac_pcm16(mrc_handle* h, int64_t n_files, const uint8_t* buf, const int64_t* file_offset, int16_t* out,
                         int64_t out_cap, int64_t* sample_offset, int32_t* n_channels);
/* Device time of the last mrc_decode_pac_pcm16 call (ms): [0] host -> device copy, [1] unpack kernel, [2] synthesis
 * (decode_kernel launches + interleaved pcm16), [3] device -> host copy. */
int mrc_get_decode_ms(mrc_handle* h, double* ms /*[4]*/);

/* mrc_pac_nmr: the noise-to-mask ratio (NMR) of n_files whole `.pac` files against the source they were coded from, in
 * ONE call, measured with the codec's own masking model.  The files are read as mrc_decode_pac_pcm16 reads them (host
 * memory; the same parameter checks against the handle and the same error texts; a stereo file of more than one block
 * is joint blocks followed by Close()'s two non-joint chunks).  File f's source channel c is
 * src[src_offset[f] + c * src_stride[f] + t] for t < src_frames[f] and zero beyond: the WAV's own samples as 16-bit
 * codes, without the prior hop (the layout of the fixtures and of cli.read_wav_pcm).  The library cannot see how long
 * src is: the caller must hold a channel row of src_frames[f] samples for every channel the file's header names (the
 * Python binding checks the rows against each header).  Block i of shape (a_i, b_i)
 * covers [p_i, p_i + a_i + b_i) of the channel's padded source (n_mdct_lines zeros, the samples, zeros),
 * p_i = a_0 + ... + a_{i-1}.  For every entry e = (block, channel), with X the windowed MDCT lines of the source block
 * (mrc_mdct, apply_window = 1), X^ the decoded lines of the channel before the IMDCT (dequantised, divided by the
 * overall scale level, L / R rebuilt in M/S bands) and T the masked threshold of the source block in dB SPL
 * (psychoac.py:134-173, the handle's MRC_OPT_EXACT_SPREAD), band j gives
 *   noise_j = sum_k 4 (X[k] - X^[k])^2,  mask_j = sum_k 10^((T[k] - 96) / 10),  r_j = noise_j / mask_j
 * (r_j = 0 where mask_j is +inf: the top lines from ~80 kHz on).  Per file:
 *   nmr_max_db      10 log10 of the largest r_j over all entries and bands;
 *   nmr_total_db    10 log10(sum_e b_e mean_j(r_j) / sum_e b_e): band-averaged ratios weighted by the block's b;
 *   disturbed_blocks  blocks in which some channel has a band with r_j > 1;  n_blocks.
 * A file without blocks gives -inf, -inf, 0, 0; r_j = 0 everywhere gives -inf.  Entries are ordered by file, block,
 * channel; file f's are [entry_offset[f], entry_offset[f + 1]).  entry_shape (NULL or [entry_cap][2]: a, b) and
 * band_noise / band_mask (both NULL or both [entry_cap][MRC_MAX_BANDS], zeros past a block's band count) return the
 * entries.  If any of them is asked for and entry_cap is too small, the call returns MRC_ERR_NOMEM after reading only
 * the headers and chunk lengths on the host (no device call of any kind), fills entry_offset [n_files + 1] and
 * n_blocks [n_files] and writes nothing else.  entry_shape and the band arrays are written only by a call that succeeds.  MRC_ERR_INVALID, the text
 * naming the file: a file the decoder refuses; a negative src_offset, src_stride or src_frames; a stride below
 * src_frames for a stereo file; a NULL src with src_frames > 0.  Results are bit-identical from call to call and
 * whatever other files share the call.  Device memory: ~16 bytes per source line analysed (distinct source, position
 * and shape: the rungs of a ladder share one analysis) plus the padded int16 sources. */
int mrc_pac_nmr(mrc_handle* h, int64_t n_files, const uint8_t* buf, const int64_t* file_offset /*[n_files+1]*/,
                const int16_t* src, const int64_t* src_offset /*[n_files]*/, const int64_t* src_stride /*[n_files]*/,
                const int64_t* src_frames /*[n_files]*/,
                double* nmr_max_db, double* nmr_total_db, int64_t* disturbed_blocks, int64_t* n_blocks /*[n_files]*/,
                int64_t* entry_offset /*[n_files+1]*/, int64_t entry_cap,
                int32_t* entry_shape /* NULL or [entry_cap][2]: a, b */,
                double* band_noise /* NULL or [entry_cap][MRC_MAX_BANDS] */,
                double* band_mask /* NULL or [entry_cap][MRC_MAX_BANDS] */);
/* Device time of the last mrc_pac_nmr call (ms): [0] host -> device copy, [1] unpack kernel, [2] source analysis
 * (padding, MDCT and masked thresholds), [3] NMR kernels + device -> host copy. */
int mrc_get_nmr_ms(mrc_handle* h, double* ms /*[4]*/);

/* ---- resident `.pac` store: sample windows of many files, decoded into device tensors ----
 * Upload the files once, then cut windows from them for ever: no file byte crosses PCIe again, a call parses and
 * synthesises only the blocks its windows overlap, and the result is written where the caller wants it on the device, in the
 * format the caller wants.
 *
 * mrc_pac_index (host only: no GPU, no handle): headers, chunk lengths and each chunk's block-switch bits of ONE `.pac` file
 * -> where every block lies.  cfg: n_short and blksw_bits_a / _b are read from it; sample_rate, n_mdct_lines, n_scale_bits
 * and n_mant_size_bits must equal the file's (MRC_ERR_INVALID naming the parameter, as mrc_decode_pac_pcm16 words it).
 * Block i: block_start[i] = a_0 + .. + a_{i-1} (its position in the padded plane: n_mdct_lines zeros, the samples, zeros),
 * block_a / block_b [i], chunk_offset[i * n_channels + c] (byte offset of the chunk's 4-byte length in buf).
 * n_samples = max(0, block_start[last] + a_last + b_last - n_mdct_lines): what mrc_decode_pac_pcm16 returns per channel.
 * block_cap too small (or an array NULL while the file has blocks): MRC_ERR_NOMEM with n_channels, n_blocks and n_samples
 * filled and the arrays untouched.  Refusals (MRC_ERR_INVALID, the text from mrc_last_error(NULL)) are exactly those of
 * mrc_decode_pac_pcm16's host plan: no header, a truncated chunk, a chunk without a block shape, a chunk count that is no
 * multiple of the channels, a block whose chunks differ in shape. */
int mrc_pac_index(const mrc_config* cfg, const uint8_t* buf, int64_t len, int32_t* n_channels, int64_t* n_blocks,
                  int64_t* n_samples, int64_t block_cap, int64_t* block_start, int32_t* block_a, int32_t* block_b,
                  int64_t* chunk_offset);

typedef struct mrc_pac_store mrc_pac_store;
#define MRC_WINDOW_PCM16 0   /* int16: the codes mrc_decode_pac_pcm16 writes */
#define MRC_WINDOW_F32   1   /* (float) of the F64 value, round to nearest even */
#define MRC_WINDOW_F64   2   /* the overlap-added signed fraction before the PCM quantiser */

/* mrc_pac_store_create: n_files whole `.pac` files, file f = buf[file_offset[f], file_offset[f + 1]) in host memory, checked
 * exactly as mrc_decode_pac_pcm16 checks them (the same refusals and texts, under this function's name), copied to the
 * handle's device ONCE and indexed on the host as mrc_pac_index does.  No chunk payload is parsed.  The store belongs to h
 * and must be destroyed before it: after mrc_destroy(h) every call on the store except mrc_pac_store_destroy returns
 * MRC_ERR_INVALID (text from mrc_last_error(NULL)), its device memory having gone with the handle.  Calls on one handle,
 * those on its stores included, are serialised by the caller.  Errors of the store's calls are read with mrc_last_error(h).
 * mrc_pac_store_destroy(NULL) does nothing.
 * mrc_pac_store_info: the file count, per file (each array NULL or [n_files]) its channels, samples per channel and
 * blocks, and the device memory the store holds. */
int mrc_pac_store_create(mrc_handle* h, int64_t n_files, const uint8_t* buf, const int64_t* file_offset /*[n_files+1]*/,
                         mrc_pac_store** out);
void mrc_pac_store_destroy(mrc_pac_store* s);
int mrc_pac_store_info(mrc_pac_store* s, int64_t* n_files, int32_t* n_channels /*NULL or [n_files]*/,
                       int64_t* n_samples /*NULL or [n_files]*/, int64_t* n_blocks /*NULL or [n_files]*/,
                       int64_t* device_bytes);
/* mrc_pac_store_decode_window: out[i][c][t] (DEVICE memory, [n_items][n_channels_out][window] of the format's type) = sample
 * start[i] + t of channel c of file file[i], in the coordinates of mrc_decode_pac_pcm16's output (the MDCT's first
 * n_mdct_lines samples already dropped), and exactly +0.0 / 0 where start[i] + t lies outside [0, n_samples): start may be
 * negative or past the end.  MRC_WINDOW_PCM16 values are bit-identical to that slice of mrc_decode_pac_pcm16's output,
 * MRC_WINDOW_F64 values to the same slice of the overlap-added plane the 16-bit codes are taken from (each sample is the
 * same at most two contributions added to zero), MRC_WINDOW_F32 is that value converted once.  A file of n_channels_out
 * channels maps one to one, a mono file in a two-channel call is written to both channels, a stereo file in a one-channel
 * call is refused.  An item's result does not depend on what shares the call, on the order of the items or on the slab size.
 * Work follows the windows, not the files: only the chunks of blocks that overlap a window are parsed -- block i of a file
 * iff block_start[i] < start + window + n_mdct_lines and block_start[i] + a_i + b_i > start + n_mdct_lines -- so a damaged
 * chunk inside a window gives MRC_ERR_INVALID (file, byte offset in the file, what the parser met; out is then unspecified)
 * while a damaged chunk outside every window of the call is never read and never reported.  An item that needs no block is
 * zeros.  MRC_ERR_INVALID naming the argument, before any device work: file[i] outside the store, window < 0,
 * n_channels_out not 1 or 2, an unknown format, out == NULL with n_items * window > 0, a stereo file in a one-channel call
 * (the item is named).  window == 0 or n_items == 0: MRC_OK, nothing written.  The call enqueues on `stream` (NULL: the
 * handle's) and synchronises it before it returns, because the parser's error word comes back.  A call is cut into slabs
 * of whole items (MRC_OPT_STORE_SLAB_SAMPLES); the workspace is the handle's, sized by the slab and reused.
 * mrc_pac_store_stats, for the store's last mrc_pac_store_decode_window(_reduced, _mix): stats = chunks parsed, decode_kernel launches,
 * slabs, bytes of plan uploaded (no file bytes among them); ms = device time of the plan upload, the unpack kernel, the
 * synthesis (zeroing the planes + decode_kernel launches) and window_out_kernel, summed over the slabs.  After
 * mrc_pac_store_block_energy the same slots describe that call (see there). */
int mrc_pac_store_decode_window(mrc_pac_store* s, int64_t n_items, const int64_t* file /*[n_items]*/,
                                const int64_t* start /*[n_items]*/, int64_t window, int n_channels_out, int format,
                                void* out /* DEVICE [n_items][n_channels_out][window] */, void* stream);
int mrc_pac_store_stats(mrc_pac_store* s, int64_t* stats /*[4]*/, double* ms /*[4]*/);
/* mrc_pac_store_decode_window_reduced: mrc_pac_store_decode_window at 1 / rate_divisor of the files' sample rate, straight
 * from the MDCT lines: of every block the first 1 / D of the lines go through an inverse transform D times shorter, shape
 * (a, b) / D with the codec's own transition window (KBD, alpha 4) at those lengths, so the synthesis does 1 / D of the work
 * and the planes and the output take 1 / D of the bytes.  The result is the decoded signal band-limited to the new Nyquist
 * frequency by a cut on MDCT lines -- no resampling filter runs; content right next to the cut-off is attenuated and aliased
 * within a few lines of it, as such a cut does -- and it is NOT scaled.
 * rate_divisor D is 1, 2 or 4.  D = 1 is mrc_pac_store_decode_window exactly (the same kernels, the same bits).  Anything
 * else, or a D for which one of the handle's four block shapes (L,L), (L,S), (S,S), (S,L) has no reduced synthesis shape --
 * a / D and b / D whole and positive, their sum and difference divisible by 4, (a + b) / (4 D) and (a + b) / (2 D) products of
 * 2s and 3s -- is MRC_ERR_INVALID naming D and the shape, before any device work.
 * start and window count REDUCED samples.  Reduced sample m of a file is the band-limited signal at time D m + (D - 1) / 2
 * in the coordinates of mrc_decode_pac_pcm16's output: it lies (D - 1) / 2 full-rate samples AFTER full-rate sample D m
 * (half a sample at D = 2, one and a half at D = 4).  The MDCT's first n_mdct_lines / D samples are dropped as the first
 * n_mdct_lines are at full rate; a file has n_samples / D reduced samples (exact: every block length is a multiple of
 * n_short, which D divides), and samples outside [0, n_samples / D) are exactly +0.0 / 0.  Block i of a file is parsed iff
 * block_start[i] / D < start + window + n_mdct_lines / D and (block_start[i] + a_i + b_i) / D > start + n_mdct_lines / D; the
 * whole chunk of such a block is parsed (its bits are sequential).  MRC_WINDOW_F64 is the overlap-added reduced plane,
 * MRC_WINDOW_F32 that value converted once, MRC_WINDOW_PCM16 the 16-bit code of it (pcmfile.py:163-172).  Everything else --
 * the channel map, the refusals, damage inside and outside a window, the independence of item order and slab size, slabs by
 * MRC_OPT_STORE_SLAB_SAMPLES (counting reduced samples), the stream, mrc_pac_store_stats -- is mrc_pac_store_decode_window's. */
int mrc_pac_store_decode_window_reduced(mrc_pac_store* s, int rate_divisor, int64_t n_items, const int64_t* file /*[n_items]*/,
                                        const int64_t* start /*[n_items]*/, int64_t window, int n_channels_out, int format,
                                        void* out /* DEVICE [n_items][n_channels_out][window] */, void* stream);
/* mrc_pac_store_decode_window_mix: ONE channel of every item, whatever its file's channel count -- out[i][0][t] -- at
 * 1 / rate_divisor of the sample rate.  Everything not named here is mrc_pac_store_decode_window_reduced's under this
 * function's name: coordinates, rate_divisor 1 / 2 / 4 and its shape refusals, zeros outside the file, the overlap rule,
 * damage inside or outside a window, slabs, the stream, the three formats, mrc_pac_store_stats.
 * A mono file gives its one channel for every mix: the bits of the one-channel call at that divisor.
 * MRC_MIX_LEFT / MRC_MIX_RIGHT of a stereo file: bit-identical, in all three formats, to channel 0 / 1 of the two-channel
 * call at that divisor (each sample is the same at most two contributions added to zero).
 * MRC_MIX_MID of a stereo file is defined on the MDCT lines, before the inverse transform.  With l1, l2 the two streams'
 * dequantised lines of a joint block, each divided by its overall scale level: line k of the mid is l1 where the band's M/S
 * switch is set (the first stream IS (L + R) / 2; the side stream of such a band is not dequantised) and 0.5 * (l1 + l2)
 * where it is not; for the file's last block, whose two chunks are not joint, 0.5 * (x0 + x1) of the two channels' lines.
 * One inverse transform, window and overlap-add per block follow: MRC_WINDOW_F64 is that plane -- the mean of the two
 * channels' planes up to rounding, the transform being linear -- MRC_WINDOW_F32 and MRC_WINDOW_PCM16 conversions of it (the
 * 16-bit code is that of the float64 mid, not the mean of two codes).  An item's result does not depend on its company,
 * the order, the slab size or how a window is cut.
 * Work per needed block of a stereo file: one synthesis workgroup, not two; one margin plane per item.  A joint block has
 * both chunks parsed for every mix (the M/S switches and both streams are needed even for left); the last block of a
 * stereo file has two chunks parsed for MRC_MIX_MID and ONE for left / right -- the other channel's chunk is not in the
 * plan, so damage in it goes unnoticed.  chunks_parsed counts accordingly.
 * mix outside {0, 1, 2}: MRC_ERR_INVALID naming mix and its value, before any device work (out untouched).  The refusal
 * of a stereo file in a one-channel call of the two calls above is theirs alone and stays. */
#define MRC_MIX_MID   0   /* (L + R) / 2 */
#define MRC_MIX_LEFT  1
#define MRC_MIX_RIGHT 2
int mrc_pac_store_decode_window_mix(mrc_pac_store* s, int rate_divisor, int mix, int64_t n_items, const int64_t* file /*[n_items]*/,
                                    const int64_t* start /*[n_items]*/, int64_t window, int format,
                                    void* out /* DEVICE [n_items][1][window] */, void* stream);
/* mrc_pac_store_block_energy: how much of the decoded signal's energy each block of the selected files holds, from the MDCT
 * lines alone -- no inverse transform, no plane, no output tensor.  The windowed MDCT with the codec's transition windows is
 * an orthogonal lapped transform (mdct.py: forward factor 2 / N, inverse factor 2), so with x^ a block's decoded lines
 *   sum_t x[t]^2 = sum_i (a_i + b_i) sum_k x^_i[k]^2
 * over the whole overlap-added plane of a channel (the MDCT's first n_mdct_lines samples included), and the reduced plane of
 * mrc_pac_store_decode_window_reduced obeys the same identity with the lines it keeps.  An entry is a (block, channel of the
 * file) under MRC_MIX_EACH and a block under MRC_MIX_MID:
 *   energy = ((a + b) / D) * sum_{k < (a + b) / (2 D)} x^[k]^2
 * x^[k] the line mrc_pac_store_decode_window(_reduced) transforms for that channel (dequantised, divided by the overall
 * scale, L / R rebuilt in M/S bands; the full shape's bands, a band that straddles the cut counted on its lines below it),
 * or the mid's line as mrc_pac_store_decode_window_mix defines it; a mono file under MRC_MIX_MID gives its own channel.
 * Where the energy lies in time is for the caller to say: block i is centred on its overlap halves, so it is usually
 * spread over [block_start + a / 2, block_start + a + b / 2) of the padded plane (mrcaudiocodec_amd/levels.py).
 * file [n_sel]: indices into the store, in any order, repeats allowed; NULL with n_sel = the store's file count: every file
 * in order.  Entries are ordered by selected file, block, channel; selection k's are [entry_offset[k], entry_offset[k + 1]).
 * entry_block (NULL or [entry_cap][3]): block_start, a, b of each entry's block at full rate, block_start in the padded plane
 * as mrc_pac_index counts it.  energy: HOST memory [entry_cap].
 * The order of every sum is fixed (lane l of a wave adds lines l, l + 64, ... in ascending order, then one fixed tree over
 * the 64 lanes, then one multiplication; no atomics): results are bit-identical from call to call and do not depend on the
 * order of the selection, on which files share the call or on the slab size.
 * MRC_ERR_INVALID naming the argument, before any device work: mix not MRC_MIX_EACH or MRC_MIX_MID; rate_divisor not 1, 2
 * or 4, or one of the handle's block shapes without a reduced shape (the refusal of mrc_pac_store_decode_window_reduced
 * under this function's name); a file index outside the store; file NULL with another n_sel; entry_offset NULL.
 * entry_cap below the entry count: MRC_ERR_NOMEM with entry_offset filled, nothing else written and no device work.
 * ALL chunks of the selected files are parsed: a damaged chunk gives MRC_ERR_INVALID with file (its index in the store), byte
 * offset and what the parser met, as a window over that block does; energy and entry_block are then unspecified.
 * The call runs in slabs of whole blocks, in entry order, whose b / D sum to at most MRC_OPT_STORE_SLAB_SAMPLES (at least one
 * block; 0: one slab), in the handle's workspace, and synchronises `stream` (NULL: the handle's) after each slab, because
 * the parser's error word comes back.  mrc_pac_store_stats then describes this call: stats = chunks parsed,
 * block_energy_kernel launches (one per slab and (shape, kind) group with blocks), slabs, bytes of plan uploaded; ms = plan
 * upload, unpack kernel, block_energy_kernel, 0. */
#define MRC_MIX_EACH  3   /* mrc_pac_store_block_energy, _band_energy_window: every channel of the file, an entry each */
int mrc_pac_store_block_energy(mrc_pac_store* s, int rate_divisor, int mix, int64_t n_sel,
                               const int64_t* file /* [n_sel], NULL: every file in order */,
                               int64_t* entry_offset /* [n_sel + 1] */, int64_t entry_cap,
                               int64_t* entry_block /* NULL or [entry_cap][3]: block_start, a, b (full rate, padded plane) */,
                               double* energy /* HOST [entry_cap] */, void* stream);
/* mrc_synthesis_shape: the rule above for one block shape (a, b) and divisor, on the host alone (no handle, no device):
 * MRC_OK if blocks of shape (a, b) have a synthesis shape (a, b) / rate_divisor, else MRC_ERR_INVALID with the reason, the
 * divisor and the shape in mrc_last_error(NULL).  rate_divisor is any positive number here: 1 asks whether (a, b) itself
 * has an inverse transform. */
int mrc_synthesis_shape(int a, int b, int rate_divisor);
/* mrc_band_line_ranges: which MDCT lines of a block of shape (a, b) a set of frequency bands holds, on the host alone (no
 * handle, no device).  With halfN = (a + b) / 2, line k lies at f_k = (k + 0.5) * ((sample_rate / halfN) / 2.) -- the
 * reference's own expression, in float64 (psychoac.py:94) -- and line_lo[q] is the number of lines with f_k < edge_hz[q]
 * (its comparison, psychoac.py:99).  Band q, [edge_hz[q], edge_hz[q + 1]), holds lines [line_lo[q], line_lo[q + 1]), which
 * may be none: a short block has few lines, and a band narrower than its line spacing that no line centre falls into is
 * empty there.  Lines below edge_hz[0] or at or above edge_hz[n_bands] belong to no band.  MRC_ERR_INVALID naming the
 * argument (mrc_last_error(NULL)): n_bands outside 1..MRC_MAX_STORE_BANDS, an edge that is not finite, edge_hz[0] < 0,
 * edges not strictly increasing, a shape mrc_synthesis_shape(a, b, 1) refuses. */
#define MRC_MAX_STORE_BANDS 256
int mrc_band_line_ranges(double sample_rate, int a, int b, int n_bands, const double* edge_hz /*[n_bands+1]*/,
                         int32_t* line_lo /*[n_bands+1]*/);
/* mrc_pac_store_band_energy_window: a band-energy spectrogram of every item, from the MDCT lines alone -- no inverse
 * transform, no plane, no STFT.  out[i][c][q][j] (DEVICE memory, [n_items][n_channels_out][n_bands][n_frames], float or
 * double) is the energy of band q that frame j = [start[i] + j hop, start[i] + (j + 1) hop) of file file[i] holds, in the
 * full-rate coordinates of mrc_pac_store_decode_window:
 *   B_n[c][q]       = sum of x^_n,c[k]^2 over the lines k of band q (mrc_band_line_ranges for block n's shape, the
 *                     handle's sample rate), x^ the lines mrc_pac_store_block_energy squares;
 *   tile_n          = [p_n + a_n / 2 - L, p_n + a_n + b_n / 2 - L), L = n_mdct_lines: tiles abut and partition time;
 *   out[i][c][q][j] = sum_n ov2(n, j) * B_n[c][q],   ov2 = 2 |tile_n and frame j|, an exact integer on doubled coordinates:
 * a block's (a + b) B spread evenly over its (a + b) / 2 samples is 2 B per sample.  Summed over bands [0, fs / 2] and over
 * frames that cover every tile this is the decoded signal's sum of squares (mrc_pac_store_block_energy's identity); a
 * frame's value is local to within the blocks it cuts, and a band carries its neighbours' window leakage as any
 * spectrogram does.  A band that holds no line of a block's shape reads 0 there.  A frame outside every tile is +0.0.
 * mix: MRC_MIX_EACH with n_channels_out 1 or 2 (the channel map and the stereo-in-one-channel refusal of
 * mrc_pac_store_decode_window), or MRC_MIX_MID / _LEFT / _RIGHT with n_channels_out 1 (the lines of
 * mrc_pac_store_decode_window_mix; a mono file gives its own channel).  format: MRC_WINDOW_F32 or MRC_WINDOW_F64.
 * Every bit is defined.  B is a left fold from +0.0 over k ascending, each square rounded once, then added (no fused
 * multiply-add).  A frame's value is a left fold from +0.0, over the item's blocks in ascending order with ov2 > 0, of
 * (double)ov2 * B; MRC_WINDOW_F32 is one conversion of it.  No atomics: results do not depend on the order of the items,
 * on what shares the call, on the slab size or on the launch grid.
 * Block n of an item is parsed iff its tile overlaps [start, start + n_frames hop) -- fewer blocks than a window of that
 * length decodes; nothing is synthesised.  Damage inside such a block gives MRC_ERR_INVALID with file, byte offset and
 * the parser's words; damage elsewhere is never read.  n_items = 0 or n_frames = 0: MRC_OK, nothing written.
 * MRC_ERR_INVALID naming the argument, before any device work: a mix outside the four, n_channels_out wrong for the mix, a
 * format other than F32 / F64, n_frames < 0, hop < 1, n_frames hop above 2^62, the refusals of mrc_band_line_ranges, a
 * file index outside the store, out NULL with output to write, a stereo file in a one-channel MRC_MIX_EACH call.
 * Slabs are whole items whose n_frames hop sum to at most MRC_OPT_STORE_SLAB_SAMPLES (one item at least; 0: one slab);
 * `stream` (NULL: the handle's) is synchronised after each.  mrc_pac_store_stats then describes this call: stats = chunks
 * parsed, band_energy_kernel launches (one per slab and (shape, kind) group with blocks), slabs, bytes of plan uploaded;
 * ms = plan upload, unpack kernel, band sums (band_energy_kernel), frame assembly (band_frames_kernel). */
int mrc_pac_store_band_energy_window(mrc_pac_store* s, int mix, int64_t n_items, const int64_t* file /*[n_items]*/,
                                     const int64_t* start /*[n_items]*/, int64_t n_frames, int64_t hop, int n_bands,
                                     const double* edge_hz /*[n_bands+1]*/, int n_channels_out, int format,
                                     void* out /* DEVICE [n_items][n_channels_out][n_bands][n_frames] */, void* stream);
/* mrc_filterbank_line_weights: the weights with which the MDCT lines of a block of shape (a, b) enter a bank of triangular
 * filters (mel, Bark, ERB, ...), on the host alone (no handle, no device).  n_filters in 1..MRC_MAX_STORE_BANDS; point_hz
 * [n_filters + 2] finite, point_hz[0] >= 0, strictly increasing (points above Nyquist are allowed).  Filter q is the
 * triangle with feet p0 = point_hz[q], p2 = point_hz[q + 2] and peak 1 at p1 = point_hz[q + 1]; norm is
 * MRC_FILTER_NORM_NONE or MRC_FILTER_NORM_SLANEY, which multiplies every weight of filter q by 2.0 / (p2 - p0).
 * With halfN = (a + b) / 2 and d = (sample_rate / halfN) / 2., line k occupies [e_k, e_{k+1}), e_k = k * d (its centre is
 * mrc_band_line_ranges' f_k), and its weight is the triangle's MEAN over that interval, so that a filter narrower than a
 * block's line spacing still reads its share of the line it lies in -- no filter is empty below the last line's upper edge:
 *   line_lo[q] = #{k < halfN : e_{k+1} <= p0},  line_hi[q] = #{k < halfN : e_k < p2};  for line_lo[q] <= k < line_hi[q],
 *   with f0 = e_k and f1 = e_{k+1}, in float64 and exactly this order of operations (no fused multiply-add):
 *     u0 = max(f0, p0); u1 = min(f1, p1); rise = u1 > u0 ? ((0.5 * (u0 + u1) - p0) / (p1 - p0)) * (u1 - u0) : 0.0
 *     v0 = max(f0, p1); v1 = min(f1, p2); fall = v1 > v0 ? ((p2 - 0.5 * (v0 + v1)) / (p2 - p1)) * (v1 - v0) : 0.0
 *     w  = (rise + fall) / d;             MRC_FILTER_NORM_SLANEY:  w = w * (2.0 / (p2 - p0))
 * weight holds the rows one after the other, filter 0's line_hi[0] - line_lo[0] weights first; *n_weights is their number.
 * weight NULL: sizes only (line_lo, line_hi and *n_weights are written, weight_cap is not looked at).
 * MRC_ERR_INVALID naming the argument (mrc_last_error(NULL)): n_filters outside 1..MRC_MAX_STORE_BANDS, a point that is
 * not finite, point_hz[0] < 0, points not strictly increasing (with the index), norm outside {0, 1}, a shape
 * mrc_synthesis_shape(a, b, 1) refuses, weight_cap below *n_weights with weight given. */
#define MRC_FILTER_NORM_NONE 0
#define MRC_FILTER_NORM_SLANEY 1
int mrc_filterbank_line_weights(double sample_rate, int a, int b, int n_filters, const double* point_hz /*[n_filters+2]*/,
                                int norm, int32_t* line_lo /*[n_filters]*/, int32_t* line_hi /*[n_filters]*/,
                                int64_t weight_cap, double* weight /* rows one after the other; NULL: sizes only */,
                                int64_t* n_weights);
/* mrc_pac_store_filterbank_window: mrc_pac_store_band_energy_window with a bank of triangular filters in place of the
 * rectangular bands -- a mel (Bark, ERB) spectrogram of every item from the MDCT lines alone.  out[i][c][q][j] (DEVICE
 * memory, [n_items][n_channels_out][n_filters][n_frames]):
 *   F_n[c][q]       = the left fold from +0.0 over k = line_lo[q] .. line_hi[q] - 1 ascending of w_q[k] * (x^[k] * x^[k]),
 *                     w_q, line_lo and line_hi those of mrc_filterbank_line_weights for block n's shape and the handle's
 *                     sample rate, x^ the lines mrc_pac_store_band_energy_window squares: the square is rounded once, the
 *                     product is rounded once, then it is added (no fused multiply-add);
 *   out[i][c][q][j] = sum_n (double)ov2(n, j) * F_n[c][q], the band call's frames, tiles and fold with F in B's place.
 * Items, frames, mixes, channels, formats, extreme starts, damage, the "nothing to write" cases, slabs and
 * mrc_pac_store_stats are the band call's: stats[1] counts filterbank_energy_kernel launches, ms[2] is that kernel's time.
 * Every bit is defined; results do not depend on the order of the items, on what shares the call, on the slab size or on
 * the launch grid.  This is not an STFT mel spectrogram: its time resolution is the block tile's and its frequency
 * resolution the block's line spacing.  Log compression is the caller's.
 * MRC_ERR_INVALID naming the argument, before any device work (out untouched): the band call's own refusals with the
 * refusals of mrc_filterbank_line_weights in the place of mrc_band_line_ranges'. */
int mrc_pac_store_filterbank_window(mrc_pac_store* s, int mix, int64_t n_items, const int64_t* file /*[n_items]*/,
                                    const int64_t* start /*[n_items]*/, int64_t n_frames, int64_t hop, int n_filters,
                                    const double* point_hz /*[n_filters+2]*/, int norm, int n_channels_out, int format,
                                    void* out /* DEVICE [n_items][n_channels_out][n_filters][n_frames] */, void* stream);
/* mrc_resample_taps: the filter of mrc_pac_store_decode_window_resampled, on the host alone (no handle, no device).
 * up / down is the output rate over the input rate; the library reduces it by the gcd.  After reduction 1 <= up, down <= 1024,
 * up != down, down <= 8 up and up <= 8 down; zeros in [1, 64]; rolloff in [0.5, 1]; anything else is MRC_ERR_INVALID naming
 * the argument (mrc_last_error(NULL)).
 *   base = min(1, up / down) * rolloff        the cut-off as a fraction of the input's Nyquist frequency
 *   W    = ceil(zeros / base)                 (both in double) written to *half_width (NULL: not wanted)
 *   taps [up][2 W] (NULL: W alone is wanted): for phase p and tap j, with d = (j - W + 1) - p / up and t = base * d,
 *     taps[p][j] = base * sinc(t) * cos^2(pi t / (2 zeros))  for |t| < zeros, else 0;  sinc(t) = sin(pi t) / (pi t), 1 at t = 0
 * -- a Hann-windowed sinc with `zeros` zero crossings a side, the shape torchaudio.functional.resample uses -- evaluated in
 * long double and rounded to double once.  d is where input sample j of the row lies relative to the output sample, so
 * taps[p][j] = taps[up - p][2 W - 1 - j] for 0 < p < up and row 0 is symmetric about j = W - 1.  The limits keep a row at or
 * below 2048 taps and a table at or below 16 MiB. */
int mrc_resample_taps(int up, int down, int zeros, double rolloff, int32_t* half_width, double* taps /* NULL or [up][2 W] */);
/* mrc_pac_store_decode_window_resampled: the windows of mrc_pac_store_decode_window_reduced / _mix at up / down of THAT
 * call's rate -- 48 kHz files at 16 kHz: rate_divisor 2, up / down = 2 / 3 -- through a polyphase filter that reads the
 * float64 overlap-added planes and writes the caller's tensor; no window at the intermediate rate is written or read back.
 * mix: MRC_MIX_EACH (every channel, as mrc_pac_store_decode_window_reduced gives them, n_channels_out 1 or 2) or
 * MRC_MIX_MID / _LEFT / _RIGHT (mrc_pac_store_decode_window_mix's one channel; n_channels_out must be 1).  rate_divisor as in
 * those calls.  up, down, zeros, rolloff: mrc_resample_taps' arguments and refusals.  start and window count OUTPUT samples.
 * The intermediate signal y[m], m any integer, is the float64 signal of the existing call at that rate_divisor and mix: the
 * plane's value for 0 <= m < n_samples / rate_divisor, +0.0 everywhere else -- what MRC_WINDOW_F64 of that call gives.
 * Output sample n sits at intermediate time n down / up (full-rate time D n down / up + (D - 1) / 2).  With
 * q = floor(n down / up) and p = n down mod up (floored: n may be negative), W and taps those of mrc_resample_taps,
 *   v[n] = the left fold from +0.0 over j = 0 .. 2 W - 1 ascending of taps[p][j] * y[q - W + 1 + j],
 * every product rounded once, then added -- no fused multiply-add.  MRC_WINDOW_F64 is v, MRC_WINDOW_F32 (float) v,
 * MRC_WINDOW_PCM16 the 16-bit code of v (pcmfile.py:163-172).  Every bit is defined: nothing depends on the launch grid, on
 * the order of the items, on which items share the call or on the slab size.  A file has ceil(n_samples / D * up / down)
 * output samples that lie inside it; the filter's tails reach W up / down samples beyond either end, then all is +0.0.
 * Work follows the windows: an item needs intermediate samples floor(start down / up) - W + 1 up to and including
 * floor((start + window - 1) down / up) + W, and the blocks parsed and synthesised are those the existing call parses for
 * a window over exactly that span; an item whose span meets no block is zeros.  Slabs are whole items whose spans, each
 * counted as ceil((window - 1) down / up) + 2 W plane samples, sum to at most MRC_OPT_STORE_SLAB_SAMPLES (one item at least).
 * All arithmetic on n down is 64-bit; window <= 2^40; a start beyond +-2^52 lies beyond every file and gives zeros.
 * MRC_ERR_INVALID naming the argument, before any device work: a mix outside the four, n_channels_out other than 1 under a
 * one-channel mix, the refusals of mrc_resample_taps, and every refusal of the existing calls (rate_divisor, file indices,
 * window, format, out, a stereo file in a one-channel MRC_MIX_EACH call).  The stream, damage inside and outside a span and
 * mrc_pac_store_stats are the existing calls'; ms[3] is resample_out_kernel's time.  The filter is computed and uploaded once
 * per handle and (up, down, zeros, rolloff). */
int mrc_pac_store_decode_window_resampled(mrc_pac_store* s, int rate_divisor, int mix, int up, int down, int zeros, double rolloff,
                                          int64_t n_items, const int64_t* file /*[n_items]*/, const int64_t* start /*[n_items]*/,
                                          int64_t window, int n_channels_out, int format,
                                          void* out /* DEVICE [n_items][n_channels_out][window] */, void* stream);
/* mrc_pac_store_decode_window_sum: windows that are weighted sums of crops -- speech over noise at a drawn SNR, an event placed
 * inside a background, two utterances overlapped -- folded from the float64 overlap-added planes straight into the caller's
 * tensor; no per-term window is written.
 * Terms: item i's terms are k in [term_offset[i], term_offset[i + 1]), n_terms = term_offset[n_items]; file, start and gain are
 * [n_terms].  An item may have no terms: its row is then +0.0 / 0.
 * One term's signal: v_k[c][t] is the MRC_WINDOW_F64 value the existing call gives for (file[k], start[k]), channel c, sample
 * t, at this rate_divisor and mix.  up == down (ratio 1; zeros and rolloff are ignored): that call is
 * mrc_pac_store_decode_window_reduced under MRC_MIX_EACH and mrc_pac_store_decode_window_mix otherwise.  up != down: it is
 * mrc_pac_store_decode_window_resampled with these up, down, zeros, rolloff; start and window then count OUTPUT samples,
 * exactly as in that call.  A start may be negative or past the end (+0.0 outside the file), so "this event begins 0.3 s into
 * that background" is a start and nothing more.
 * The sum: out[i][c][t] = the left fold from +0.0, over the item's terms IN THE ORDER GIVEN, of gain[k] * v_k[c][t]; every
 * product is rounded once, then added (__dmul_rn, __dadd_rn: no fused multiply-add).  MRC_WINDOW_F64 is that sum,
 * MRC_WINDOW_F32 one conversion of it, MRC_WINDOW_PCM16 the 16-bit code of it (pcmfile.py:163-172, saturating at full scale
 * as that map does).  Every bit is defined: nothing depends on the launch grid, on the order of the ITEMS, on what shares the
 * call or on the slab size; the order of an item's TERMS is part of the definition (floating-point addition does not
 * associate).
 * Single-term identity: a one-term item with gain 1.0 equals the existing call in all three formats -- +0.0 + 1.0 * v is v
 * for every v but -0.0, and the planes and the resample fold never hold -0.0: they are sums that start from +0.0.
 * Channel map: MRC_MIX_EACH takes n_channels_out 1 or 2; a mono file's term adds to both channels of a two-channel call, a
 * stereo file's term in a one-channel call is refused, the refusal naming the term.  MRC_MIX_MID / _LEFT / _RIGHT take
 * n_channels_out == 1, with the lines of mrc_pac_store_decode_window_mix.
 * Work follows the windows, per term: a term's blocks are those the existing call parses for that (file, start, window); a
 * term that meets no block has no plane and adds nothing; a zero gain is not special, the term is parsed like any other.
 * Damage inside a term's span gives MRC_ERR_INVALID (file, byte offset, the parser's words); damage elsewhere is never read.
 * MRC_ERR_INVALID naming the argument, before any device work and with `out` untouched: every refusal of the existing calls
 * (rate_divisor and the block shapes, mix, mrc_resample_taps' arguments when up != down, file indices, window, format, out
 * NULL with output to write); term_offset NULL, term_offset[0] != 0 or term_offset decreasing; file, start or gain NULL with
 * terms present; a gain that is not finite (the term is named); up or down < 1.  n_items == 0 or window == 0: MRC_OK, nothing
 * written.
 * Slabs are runs of whole items whose TERMS' plane spans -- window, or ceil((window - 1) down / up) + 2 W when resampling, per
 * term -- sum to at most MRC_OPT_STORE_SLAB_SAMPLES (one item at least; 0: one slab), and of at most (2^31 - 1) /
 * (n_channels_out * ceil(window / 256)) items; `stream` (NULL: the handle's) is synchronised after each.
 * mrc_pac_store_stats describes the call as it does the others, the chunks those of all terms; ms[3] is sum_out_kernel's
 * time, or resample_sum_out_kernel's. */
int mrc_pac_store_decode_window_sum(mrc_pac_store* s, int rate_divisor, int mix, int up, int down, int zeros, double rolloff,
                                    int64_t n_items, const int64_t* term_offset /*[n_items+1]*/, const int64_t* file /*[n_terms]*/,
                                    const int64_t* start /*[n_terms]*/, const double* gain /*[n_terms]*/, int64_t window,
                                    int n_channels_out, int format, void* out /* DEVICE [n_items][n_channels_out][window] */,
                                    void* stream);
/* mrc_pac_store_decode_window_shaped: the rows of mrc_pac_store_decode_window_sum with the spectrum of every term changed on
 * its MDCT lines -- a telephone band for the speech term, an EQ tilt per item, frequency masks, a per-item low-pass -- one
 * multiplication per line between the dequantiser and the inverse transform that runs anyway.
 * Bands: n_bands in 1..MRC_MAX_STORE_BANDS, edge_hz [n_bands + 1] under mrc_band_line_ranges' rule (its words in the refusal),
 * band_gain [n_terms][n_bands], finite; zero and negative gains are allowed.  For a block of full shape (a, b), band q holds the
 * lines [r[q], r[q + 1]) that mrc_band_line_ranges(sample_rate, a, b, ...) gives: the FULL shape's line frequencies at every
 * rate_divisor.  At D = 2 or 4 only the first 1 / D of the lines exist; bands above them are ignored.
 * The gain: let x[k] be the line the existing call transforms for a plane -- a channel's line after ReconstructLR, or the
 * mid's line as mrc_pac_store_decode_window_mix defines it (for the non-joint last block of a stereo file under the mid,
 * 0.5 * (x0 + x1)).  This call transforms __dmul_rn(band_gain[u][q], x[k]) instead, u the term the block is decoded for and q
 * the line's band: one product, rounded once.  A line that lies in no band (below edge_hz[0], or at or above
 * edge_hz[n_bands]) is not multiplied at all.  All channels of a term share its row of gains.
 * Everything after the lines is mrc_pac_store_decode_window_sum's, unchanged: inverse transform, window, overlap-add into the
 * float64 planes, the fold of a row's terms with `gain` (with or without the resampling filter), the three formats, zeros
 * outside the file, slabs, stats, damage rules, term order, channel map, single-term identity.  Hence:
 *   All band gains 1.0: every format equals mrc_pac_store_decode_window_sum bit for bit (x * 1.0 is x).
 *   All band gains of a term the same power of two 2^e: the term's float64 window is 2^e times its unshaped float64 window, bit
 *   for bit -- scaling by a power of two commutes with every rounding of the transform as long as nothing goes subnormal
 *   (checked on the host for D = 1, 2, 4 and 0.25, -2, 2^-20 on every block shape; a coded file's smallest nonzero line is of
 *   the order of 1e-10).
 *   The planes never hold -0.0: they remain sums that start from +0.0.
 * Not a filter in the LTI sense: per-line gains on a lapped transform leave the time-domain aliasing of adjacent blocks
 * uncancelled where neighbouring lines get different gains.  Smooth gain curves are clean; a brick-wall edge leaves a small
 * aliasing residue near the edge frequency (DESIGN.md has measured figures).
 * MRC_ERR_INVALID naming the argument, before any device work and with `out` untouched: every refusal of
 * mrc_pac_store_decode_window_sum; n_bands out of range; mrc_band_line_ranges' refusals of edge_hz; edge_hz or band_gain NULL
 * with terms present; a band gain that is not finite (the term and the band are named).
 * Per slab the line-to-band tables (a uint16 per line of each block shape), the slab's rows of band_gain and one term index per
 * decoded block go up with the plan: no further copy, no further synchronisation.  The existing entry points do not come
 * through the shaped kernels. */
int mrc_pac_store_decode_window_shaped(mrc_pac_store* s, int rate_divisor, int mix, int up, int down, int zeros, double rolloff,
                                       int n_bands, const double* edge_hz /*[n_bands+1]*/,
                                       const double* band_gain /*[n_terms][n_bands]*/, int64_t n_items,
                                       const int64_t* term_offset /*[n_items+1]*/, const int64_t* file /*[n_terms]*/,
                                       const int64_t* start /*[n_terms]*/, const double* gain /*[n_terms]*/, int64_t window,
                                       int n_channels_out, int format, void* out /* DEVICE [n_items][n_channels_out][window] */,
                                       void* stream);
/* mrc_pac_store_decode_window_speeds: the rows of mrc_pac_store_decode_window_shaped (rows of terms, optional band gains) in
 * which every term is read at a ratio of its own, chosen from a short list the call carries -- speed perturbation (each
 * utterance at 0.9x, 1.0x or 1.1x, drawn per item) in one call, and mixtures whose speech term is sped up and whose noise term
 * is not.  Term k is read at ratio r = ratio_of[k]: ratio_up[r] / ratio_down[r] of the rate 1 / rate_divisor; zeros and
 * rolloff are shared by every non-unit ratio of the list.
 * One term's signal: v_k[c][t] is the MRC_WINDOW_F64 value the EXISTING call gives for (file[k], start[k]), channel c, sample
 * t, at this rate_divisor and mix, made with that term's ratio.  A ratio that does not reduce to 1: that call is
 * mrc_pac_store_decode_window_resampled with (ratio_up[r], ratio_down[r], zeros, rolloff).  A ratio that reduces to 1: it is the
 * call without a filter, mrc_pac_store_decode_window_reduced under MRC_MIX_EACH and mrc_pac_store_decode_window_mix otherwise
 * (zeros and rolloff are not looked at if every ratio is such).  With band gains (n_bands > 0) v_k is the value of
 * mrc_pac_store_decode_window_shaped's one-term row at gain 1.0 with band_gain's row k and that ratio.  start[k] and window
 * count output samples AT THE TERM'S OWN RATIO, exactly as in those calls: a term at 10 / 11 of the rate (speed 1.1) covers
 * 1.1 times the source time that a unit term of the same window covers.
 * The row is mrc_pac_store_decode_window_sum's fold: out[i][c][t] = the left fold from +0.0, over the item's terms in the order
 * given, of gain[k] * v_k[c][t], every product rounded once, then added (__dmul_rn, __dadd_rn); MRC_WINDOW_F32 and
 * MRC_WINDOW_PCM16 are conversions of that sum; channel map, zeros outside the file and damage rules are unchanged.  Hence,
 * bit for bit: a one-term row at gain 1.0 equals the existing single-ratio call in all three formats; a call whose terms all
 * name one ratio equals mrc_pac_store_decode_window_sum / _shaped with that ratio, whatever else the list holds; nothing
 * depends on the launch grid, on the order of the items, on what shares the call or on the slab size.
 * n_bands == 0: no band gains, edge_hz and band_gain must be NULL.
 * MRC_ERR_INVALID naming the argument, before any device work and with `out` untouched: every refusal of
 * mrc_pac_store_decode_window_shaped (of mrc_pac_store_decode_window_sum when n_bands == 0); n_bands == 0 with edge_hz or
 * band_gain not NULL; n_ratios outside 1..MRC_MAX_STORE_RATIOS; ratio_up, ratio_down or ratio_of NULL with terms present; for
 * each ratio that does not reduce to 1, mrc_resample_taps' own words behind "ratio <index>: " -- the list is checked wherever
 * ratio_up and ratio_down are given, also in a call without terms; ratio_of[k] outside the list (the term is named).  n_items == 0 or window == 0: MRC_OK, nothing written.
 * Work follows the spans, per term: a unit-ratio term parses the blocks of [start, start + window), any other the blocks of
 * the intermediate span its filter reads; the chunks parsed are the sum of the existing calls' over the terms.
 * Slabs: every term's planes have ONE length per call, S + 4 n_mdct_lines / rate_divisor, S the largest span bound among the
 * ratios that the call's terms name (window for the unit ratio, ceil((window - 1) down / up) + 2 W otherwise); a slab is a run
 * of whole rows whose terms, EACH COUNTED AT S, sum to at most MRC_OPT_STORE_SLAB_SAMPLES (one row at least; 0: one slab), and
 * of at most (2^31 - 1) / (n_channels_out * ceil(window / 256)) rows.  Per slab the terms' ratio indices and the table of the
 * ratios go up with the plan: no further copy, no further synchronisation.
 * mrc_pac_store_stats then describes this call: stats = chunks parsed over all terms, synthesis launches, slabs, plan bytes
 * uploaded (the indices and the table included); ms[3] is resample_multi_sum_out_kernel's time.
 * All filters of the list are resolved before any is used; the handle's cache of filters (16) is emptied before the first if
 * the missing ones would not fit, never between two of one call. */
#define MRC_MAX_STORE_RATIOS 8
int mrc_pac_store_decode_window_speeds(mrc_pac_store* s, int rate_divisor, int mix, int n_ratios,
                                       const int32_t* ratio_up /*[n_ratios]*/, const int32_t* ratio_down /*[n_ratios]*/, int zeros,
                                       double rolloff, int n_bands /* 0: no band gains */, const double* edge_hz /*[n_bands+1]*/,
                                       const double* band_gain /*[n_terms][n_bands]*/, int64_t n_items,
                                       const int64_t* term_offset /*[n_items+1]*/, const int64_t* file /*[n_terms]*/,
                                       const int64_t* start /*[n_terms]*/, const double* gain /*[n_terms]*/,
                                       const int32_t* ratio_of /*[n_terms]: index into the list*/, int64_t window,
                                       int n_channels_out, int format, void* out /* DEVICE [n_items][n_channels_out][window] */,
                                       void* stream);

/* Reverberation: window terms convolved with room impulse responses before they are mixed (speech through a room over dry
 * noise), in the call that reads them -- no per-term tensor, no torch.fft.
 * THE BANK.  mrc_pac_store_set_irs gives the store a bank of n_irs impulse responses: response j is the host float64 taps
 * [ir_offset[j], ir_offset[j + 1]), ir_offset[0] == 0, each of 1..MRC_MAX_STORE_IR_TAPS finite taps (2^17: 2.7 s at 48 kHz),
 * SAMPLED AT THE OUTPUT RATE OF THE TERMS that will name it (after the rate divisor and the resample or speed ratio: the rate
 * the model sees, and the physical order -- speed, then room).  The call replaces the previous bank; n_irs == 0 drops it.  The
 * transforms of the bank's partitions (MRC_STORE_REVERB_BLOCK taps each) are computed once, on the device, by the forward
 * kernel the signal uses, and stay resident: 32 bytes of device memory per tap, a response's length rounded up to whole
 * partitions (plus the allocator's headroom of one eighth).  MRC_ERR_INVALID naming the argument, the previous bank kept:
 * n_irs < 0, ir_offset or taps NULL with responses present, ir_offset[0] != 0, a length outside the range (the response is
 * named), a tap that is not finite (its index is named).  A failed allocation is MRC_ERR_NOMEM and leaves the store WITHOUT a
 * bank.  Synchronises the handle's stream.  mrc_pac_store_ir_info: the count and (ir_len, nullable, [n_irs]) the lengths.
 *
 * THE CALL.  mrc_pac_store_decode_window_reverb takes every argument of mrc_pac_store_decode_window_speeds and ir_of [n_terms]:
 * -1, the term is not convolved, or the index of a response of the bank.
 *   Lpre     (the longest response that the call's terms name) - 1
 *   w_k      term k's dry signal: the MRC_WINDOW_F64 window the speeds call's one-term row at gain 1.0 gives for (file[k],
 *            start[k] - Lpre, window + Lpre) at the term's rate divisor, mix, ratio and band gains.  Those windows are functions
 *            of the absolute output index, so a slice of w_k is the existing window bit for bit.
 *   y_k[t]   = sum over j of h[j] * w_k[Lpre + t - j], 0 <= t < window: the wet signal of a convolved term.  Outside the file the
 *            dry signal is zero as ever, so the wet signal rings len(h) - 1 samples past the file's end, and a window placed in
 *            that tail reads it.
 *   row i    the left fold from +0.0, over its terms in the order given, of gain[k] * (y_k | the dry window), every product
 *            rounded once, then added: mrc_pac_store_decode_window_sum's rule.  MRC_WINDOW_F32 / _PCM16 convert that sum.
 * Bit for bit: a term with ir_of -1 contributes its existing window; a row none of whose terms is convolved equals
 * mrc_pac_store_decode_window_speeds on the same arguments in all three formats (a call without any convolved term IS that
 * call).  A convolved term is computed by overlap-save in float64 -- a hop of B = MRC_STORE_REVERB_BLOCK samples, transforms of
 * N = 2 B points, the segments anchored at the term's own window start -- and is defined to a tolerance, the transform's
 * rounding being the implementation's: |error| <= K 2^-52 log2(N) sum|h| max|w_k| per term, times |gain|, K measured in
 * tests/test_gpu_store_reverb.py.  But to the bit it does not depend on the order of the items, on what shares the call, on
 * the slab size, on the response's index or company in the bank, and repeats from call to call.  A two-channel term's channels
 * ride as the real and imaginary part of one transform (h is real); a one-channel term leaves the imaginary part zero.
 * MRC_ERR_INVALID naming the argument, before any device work and with `out` untouched: every refusal of the speeds call;
 * ir_of NULL with terms present; an index below -1 or outside the bank (the term is named); an index >= 0 while the store has
 * no bank; window + Lpre beyond 2^40.  n_items == 0 or window == 0: MRC_OK, nothing written.
 * Slabs: a run of whole rows whose terms, each counted at window + Lpre, sum to at most MRC_OPT_STORE_SLAB_SAMPLES (one row at
 * least; 0: one slab).  Per slab the existing machinery decodes the terms, in one slab of its own whatever their intermediate
 * spans (planes of up to `down / up` times the slab under a resample ratio), into a scratch buffer the handle owns (8 bytes per
 * sample and output channel), then reverb_forward_kernel and reverb_fold_kernel run on it on the same stream; the spectra
 * of the convolved terms' segments take 32 bytes per sample of window + len(h) rounded up to whole blocks.
 * mrc_pac_store_stats then describes the whole call (the chunks are those of the lengthened spans; ms[3] includes the two
 * reverb kernels); mrc_pac_store_reverb_ms gives those two apart: ms[0] reverb_forward_kernel, ms[1] reverb_fold_kernel (zeros
 * after a call without a convolved term). */
#ifndef MRC_STORE_REVERB_BLOCK   /* (a build-time experiment may set 2048: transforms of 4096 points, 144 KiB of LDS) */
#define MRC_STORE_REVERB_BLOCK 1024
#endif
#define MRC_MAX_STORE_IR_TAPS (1 << 17)
int mrc_pac_store_set_irs(mrc_pac_store* s, int64_t n_irs, const int64_t* ir_offset /*[n_irs+1]*/, const double* taps /* HOST */);
int mrc_pac_store_ir_info(mrc_pac_store* s, int64_t* n_irs, int64_t* ir_len /*[n_irs], nullable*/);
int mrc_pac_store_decode_window_reverb(mrc_pac_store* s, int rate_divisor, int mix, int n_ratios,
                                       const int32_t* ratio_up /*[n_ratios]*/, const int32_t* ratio_down /*[n_ratios]*/, int zeros,
                                       double rolloff, int n_bands /* 0: no band gains */, const double* edge_hz /*[n_bands+1]*/,
                                       const double* band_gain /*[n_terms][n_bands]*/, int64_t n_items,
                                       const int64_t* term_offset /*[n_items+1]*/, const int64_t* file /*[n_terms]*/,
                                       const int64_t* start /*[n_terms]*/, const double* gain /*[n_terms]*/,
                                       const int32_t* ratio_of /*[n_terms]: index into the list*/,
                                       const int32_t* ir_of /*[n_terms]: -1 or index into the bank*/, int64_t window,
                                       int n_channels_out, int format, void* out /* DEVICE [n_items][n_channels_out][window] */,
                                       void* stream);
int mrc_pac_store_reverb_ms(mrc_pac_store* s, double* ms /*[2]*/);

/* Short-time Fourier transforms of rows: the features a pretrained front end expects (torch.stft's numbers: 400-point Hann at
 * hop 160 with 80 mel filters at 16 kHz; 25 ms frames padded to 512 points; 1024 points at hop 480 at 48 kHz) of ANY row the store
 * can make, in the call that reads it -- no waveform tensor, no torch.stft, no mel matmul.
 * THE ROW.  mrc_pac_store_stft_window takes every argument of mrc_pac_store_decode_window_reverb up to and including ir_of,
 * unchanged in order and meaning.  Row i's signal x_i[c][t], 0 <= t < L = (n_frames - 1) hop + n_fft, is the MRC_WINDOW_F64 row
 * that call gives on the same row arguments with window = L, bit for bit: terms, gains, ratios, band gains, rooms, the channel
 * map and zeros outside the file all hold as they do there.  There is no padding mode: start is sample 0 of frame 0.  A
 * caller who wants centred frames starts n_fft / 2 earlier and reads REAL signal there (zeros before the file's start), where
 * torch.stft(center=True) reflects the crop at its own ends: the two differ in the first and last frames that reach past a crop.
 * THE TRANSFORM.  X[m][k] = sum over n < n_fft of g[n] x[m hop + n] e^{-2 pi i k n / n_fft}, 0 <= k <= n_fft / 2, g = frame_window
 * as given (the caller builds Hann, Hamming, or 400 taps padded to 512: the library holds no window types); the product g x is
 * rounded once.  The transform's rounding is the implementation's (one complex transform of n_fft / 2 points per frame in
 * float64, radices 4, 2, 3, 5, twiddles rounded once from long double): |X - exact| <= K 2^-52 log2(n_fft) ||g x_m||_2 per
 * bin, K measured in tests/test_gpu_store_stft.py.
 *   MRC_STFT_COMPLEX  out[i][c][k][m][2] = (re, im) of X.
 *   MRC_STFT_POWER    out[i][c][k][m] = P = re re + im im, each product rounded once, then added, no FMA: given X, bit-defined.
 *   MRC_STFT_BANK     out[i][c][q][m] = E: row q of bank [n_filters][n_fft / 2 + 1] is used on its support [lo_q, hi_q), its
 *                     first to its last nonzero entry; E is the left fold from +0.0, in ascending k, of bank[q][k] P[m][k],
 *                     each product rounded once, then added (__dmul_rn, __dadd_rn); a row of zeros gives +0.0.  Given P,
 *                     bit-defined.  The caller's matrix is taken as it is (torchaudio's, librosa's, a model's own).
 * MRC_WINDOW_F64 is the value, MRC_WINDOW_F32 one conversion of it.  n_fft: even, 16..MRC_MAX_STFT_POINTS, no prime factor other
 * than 2, 3 and 5.  hop >= 1 with no upper bound: frames may leave gaps.
 * To the bit a result does not depend on the order of the rows, on what else shares the call, on the slab size, on the launch
 * grid nor, for the filter values, on which filters share the call (their index and their number), and it repeats from call to
 * call: frame m of a row is computed from that frame's n_fft samples alone (no two frames share a transform).  No atomics.
 * MRC_ERR_INVALID naming the argument, before any device work and with `out` untouched: every refusal of
 * mrc_pac_store_decode_window_reverb (under this call's name); n_fft outside the rule; frame_window NULL or with a tap that is
 * not finite (its index is named); n_frames < 0; hop < 1; L, or L + the longest response named - 1, beyond 2^40; an unknown mode; a format other than MRC_WINDOW_F32 /
 * _F64; mode MRC_STFT_BANK with n_filters outside 1..MRC_MAX_STORE_BANDS, a NULL bank or an entry that is not finite (named);
 * any other mode with n_filters != 0 or a bank.  n_items == 0 or n_frames == 0: MRC_OK, nothing written.
 * Slabs: runs of whole rows whose L sum to at most MRC_OPT_STORE_SLAB_SAMPLES (one row at least; 0: one slab).  Per slab the
 * reverb entry writes the rows as MRC_WINDOW_F64, in one slab of its own, into a scratch buffer the handle owns (8 bytes per
 * sample and output channel, apart from that entry's own scratch), then stft_kernel runs on the same stream.  The frame
 * window, the bank's supports and weights and the twiddle table go up once per call, before the slabs.
 * mrc_pac_store_stats then describes the whole call as the reverb call's does, ms[3] including stft_kernel;
 * mrc_pac_store_stft_ms gives that kernel apart, summed over the slabs (mrc_pac_store_reverb_ms: the reverb kernels likewise). */
#define MRC_STFT_COMPLEX 0   /* out[i][c][k][m][2]  (re, im)            */
#define MRC_STFT_POWER   1   /* out[i][c][k][m]     re^2 + im^2         */
#define MRC_STFT_BANK    2   /* out[i][c][q][m]     sum_k W[q][k] P[k]  */
#define MRC_MAX_STFT_POINTS 2048
int mrc_pac_store_stft_window(mrc_pac_store* s, int rate_divisor, int mix, int n_ratios,
                              const int32_t* ratio_up /*[n_ratios]*/, const int32_t* ratio_down /*[n_ratios]*/, int zeros,
                              double rolloff, int n_bands /* 0: no band gains */, const double* edge_hz /*[n_bands+1]*/,
                              const double* band_gain /*[n_terms][n_bands]*/, int64_t n_items,
                              const int64_t* term_offset /*[n_items+1]*/, const int64_t* file /*[n_terms]*/,
                              const int64_t* start /*[n_terms]*/, const double* gain /*[n_terms]*/,
                              const int32_t* ratio_of /*[n_terms]: index into the list*/,
                              const int32_t* ir_of /*[n_terms]: -1 or index into the bank*/, int n_fft,
                              const double* frame_window /* HOST [n_fft] */, int64_t n_frames, int64_t hop, int mode, int n_filters,
                              const double* bank /* HOST [n_filters][n_fft/2+1], mode MRC_STFT_BANK only, else NULL and 0 */,
                              int n_channels_out, int format /* MRC_WINDOW_F32 | MRC_WINDOW_F64 */, void* out /* DEVICE */,
                              void* stream);
int mrc_pac_store_stft_ms(mrc_pac_store* s, double* ms /*[1]: stft_kernel of the last call */);

/* Routes: rows of SEVERAL output channels, a gain and a response per (term, output channel), in the one call that reads the
 * terms -- an utterance through the C microphones of one room as [items][C][window]; the reverberant mixture, the dry speech
 * and the noise alone of the SAME terms as three channels.  Each term is parsed, synthesised and written to the dry scratch
 * once, whatever the number of channels it reaches.
 * THE CALL.  mrc_pac_store_decode_window_routed takes every argument of mrc_pac_store_decode_window_reverb but gain and ir_of;
 * in their place stand route_gain and route_ir, [n_terms][n_channels_out]: route_ir[k][c] is MRC_ROUTE_NONE (term k does not
 * reach channel c: no work, no contribution), -1 (dry) or the index of a response of the bank.
 * EVERY TERM GIVES ONE CHANNEL: mix is MRC_MIX_MID, _LEFT or _RIGHT, or it is MRC_MIX_EACH and every file named is mono (a
 * stereo file is then refused as a one-channel call refuses it).  n_channels_out, 1..MRC_MAX_STORE_ROUTE_CHANNELS, counts the
 * OUTPUT channels and has nothing to do with the source.
 * THE VALUE, to the bit: out[i][c] is the row mrc_pac_store_decode_window_reverb gives with n_channels_out = 1 over item i's
 * terms whose route to c is not MRC_ROUTE_NONE, in the order given, with gain[k] = route_gain[k][c] and ir_of[k] =
 * route_ir[k][c] and every other argument equal, in all three formats.  No tolerance of its own: a convolved term's bound is
 * that call's.  A row all of whose routes to a channel are absent is +0.0 there.  To the bit nothing depends on the order of
 * the rows, on what shares the call, on the slab size, on the bank's layout, on the launch grid, nor on which other channels
 * the call has, their order, or how the kernel groups them (MRC_OPT_STORE_ROUTE_GROUP).
 * WHAT IS SHARED.  A term's span is lengthened by Lpre = (the longest response any route of the call's terms names) - 1 -- a
 * longer pre-roll changes no bit -- and decoded once.  Forward transforms: ONE source per (term, distinct response LENGTH among
 * its wet routes).  A segment is zero outside [-(len(h) - 1), window) and the number of segments follows len(h), so routes
 * share spectra exactly when their responses have equal lengths (the microphones of one array); lengths are not rounded to
 * partitions for sharing.  reverb_route_fold_kernel then runs one inverse transform per (term, channel), as the reverb call
 * does per term; the channels of a workgroup that share a source load its spectra once per partition.
 * mrc_pac_store_stft_window_routed: the same row arguments, then mrc_pac_store_stft_window's own; out
 * [i][c][k | q][m]: channel c is mrc_pac_store_stft_window on that one-channel row, bit for bit in all three modes.
 * MRC_ERR_INVALID naming the argument, before any device work and with `out` untouched: every refusal of the reverb call,
 * respectively the STFT call, under this call's name; n_channels_out outside 1..MRC_MAX_STORE_ROUTE_CHANNELS; MRC_MIX_EACH with
 * a stereo file; route_gain or route_ir NULL with terms present; a gain that is not finite (term and channel named); an
 * index below MRC_ROUTE_NONE or outside the bank (term and channel named); an index >= 0 while the store has no bank;
 * window + Lpre beyond 2^40.  n_items == 0 or window == 0: MRC_OK, nothing written.
 * Slabs: the reverb call's rule, the terms counted at window + Lpre ONCE, not per channel; a slab's rows are also capped so
 * that its workgroups (rows x output blocks x channel groups) stay below 2^31.  The route records go up in the slab's one
 * staging copy.  mrc_pac_store_stats and mrc_pac_store_reverb_ms describe the call as they do the reverb call (a one-channel
 * call without an absent route and without a wet route IS the speeds call, as there).  mrc_pac_store_route_info, of the last
 * routed call, summed over its slabs: counts[0] forward segments transformed, counts[1] inverse transforms, counts[2] bytes
 * of spectra written. */
#define MRC_MAX_STORE_ROUTE_CHANNELS 16
#define MRC_ROUTE_NONE (-2)   /* the term does not reach this channel: no work, no contribution */
int mrc_pac_store_decode_window_routed(mrc_pac_store* s, int rate_divisor, int mix, int n_ratios,
                                       const int32_t* ratio_up /*[n_ratios]*/, const int32_t* ratio_down /*[n_ratios]*/, int zeros,
                                       double rolloff, int n_bands /* 0: no band gains */, const double* edge_hz /*[n_bands+1]*/,
                                       const double* band_gain /*[n_terms][n_bands]*/, int64_t n_items,
                                       const int64_t* term_offset /*[n_items+1]*/, const int64_t* file /*[n_terms]*/,
                                       const int64_t* start /*[n_terms]*/, const int32_t* ratio_of /*[n_terms]: index into the list*/,
                                       const double* route_gain /*[n_terms][n_channels_out]*/,
                                       const int32_t* route_ir /*[n_terms][n_channels_out]: MRC_ROUTE_NONE, -1 dry, or an index into the bank*/,
                                       int64_t window, int n_channels_out /* 1..16 */, int format,
                                       void* out /* DEVICE [n_items][n_channels_out][window] */, void* stream);
int mrc_pac_store_stft_window_routed(mrc_pac_store* s, int rate_divisor, int mix, int n_ratios,
                                     const int32_t* ratio_up /*[n_ratios]*/, const int32_t* ratio_down /*[n_ratios]*/, int zeros,
                                     double rolloff, int n_bands /* 0: no band gains */, const double* edge_hz /*[n_bands+1]*/,
                                     const double* band_gain /*[n_terms][n_bands]*/, int64_t n_items,
                                     const int64_t* term_offset /*[n_items+1]*/, const int64_t* file /*[n_terms]*/,
                                     const int64_t* start /*[n_terms]*/, const int32_t* ratio_of /*[n_terms]: index into the list*/,
                                     const double* route_gain /*[n_terms][n_channels_out]*/,
                                     const int32_t* route_ir /*[n_terms][n_channels_out]*/, int n_fft,
                                     const double* frame_window /* HOST [n_fft] */, int64_t n_frames, int64_t hop, int mode,
                                     int n_filters, const double* bank /* HOST [n_filters][n_fft/2+1], MRC_STFT_BANK only */,
                                     int n_channels_out /* 1..16 */, int format /* MRC_WINDOW_F32 | MRC_WINDOW_F64 */,
                                     void* out /* DEVICE */, void* stream);
int mrc_pac_store_route_info(mrc_pac_store* s, int64_t* counts /*[3]*/);

/* Spans: a term that sounds in PART of its row, with a linear fade at either end -- a row of eight utterances laid end to end
 * (packing), pieces of one file in another order, 0.5 s out of the middle of a file at 0.3 s into a 4 s background, a hole
 * cut into an utterance, a crossfade at a splice -- in the one call that reads the terms.
 * THE CALLS.  mrc_pac_store_decode_window_spans takes every argument of mrc_pac_store_decode_window_reverb, and
 * mrc_pac_store_stft_window_spans every argument of mrc_pac_store_stft_window, in that order, and right after ir_of
 *   span_first, span_len [n_terms]   in ROW samples -- output samples at the term's own ratio, as start and window are; row
 *                                    sample 0 is the row's first.  start[k] keeps its meaning: the position in the file's signal
 *                                    that stands at row sample 0, so "the piece that begins at source sample p, placed at row
 *                                    sample a" is start = p - a, span_first = a;
 *   fade_in, fade_out [n_terms]      samples of linear ramp inside the span's two ends; either may be NULL: 0.
 * ONE TERM.  With v_k[c][t] what the reverb call defines for term k (its dry window, for every integer t from -Lpre on) and
 * j = t - span_first[k]: the term is silent for j < 0 or j >= span_len[k] -- it adds nothing -- and else d_k[t] = e v_k[t],
 *   j < fade_in                e = (2 j + 1) / (2 fade_in)
 *   j >= span_len - fade_out   e = (2 (span_len - 1 - j) + 1) / (2 fade_out)
 *   otherwise                  d_k[t] is v_k[t] itself, no product;
 * e is ONE division of the two exact integers as doubles, e v ONE product (no fused multiply-add).  fade_in + fade_out <=
 * span_len, so at most one ramp holds at a sample; the half-sample ramp is symmetric and never 0 or 1, and a fade-out of F
 * samples laid over a fade-in of F samples has weights that add to 1: a linear crossfade.
 * Everything after the envelope is the reverb call's: a dry term enters the row's left fold as gain[k] * d_k[t] in the order of
 * the terms; a convolved term is y_k[t] = sum over j of h[j] d_k[t - j] -- the response acts LAST, a gated piece rings on
 * past its span; formats, channel map, zeros outside a file, damage rules and the STFT of the row are unchanged.
 * To the bit: all four arrays NULL IS the reverb / STFT call (same path, same statistics); spans that cover every sample the
 * call reads, without fades, equal it in every format; K dry terms at gain 1.0 whose spans abut and tile [0, window) give the
 * concatenation of the K existing one-term windows; nothing depends on the order of the rows, on what shares the call, on the
 * slab size or on the grid (the order of a row's terms stays part of the definition).
 * WORK FOLLOWS THE SPANS.  A_k = [span_first, span_first + span_len) cut to [-Lpre, window), Lpre the range's pre-roll (0
 * without a convolved term).  A_k empty: the term needs no block, gets no plane, parses nothing.  Else its blocks are exactly
 * those the one-term call parses for (file[k], start[k] + a0, a1 - a0) at its ratio, A_k = [a0, a1): damage outside A_k is
 * never read and never reported, and chunks_parsed of a call without convolved terms is the sum of those calls' counts.
 * Planes and slabs (no convolved term): every term's planes have ONE length per call, S' + 4 n_mdct_lines / rate_divisor, S' the
 * largest plane span of any A_k -- a1 - a0 at the unit ratio, ceil((a1 - a0 - 1) down / up) + 2 W otherwise -- not the
 * window's; a slab is a run of whole rows whose terms, each counted at S', sum to at most MRC_OPT_STORE_SLAB_SAMPLES.  A row of
 * eight abutting pieces of window / 8 counts about one window.  With a convolved term the dry scratch stays window + Lpre wide
 * per term and the slab rule is the reverb call's.
 * MRC_ERR_INVALID naming the argument and the term, before any device work and with `out` untouched: every refusal of the
 * underlying entry (under this call's name); span_first without span_len or the reverse; a fade array without spans; span_len
 * < 0 or > 2^40; |span_first| > 2^40; a negative fade; fade_in + fade_out > span_len. */
int mrc_pac_store_decode_window_spans(mrc_pac_store* s, int rate_divisor, int mix, int n_ratios,
                                      const int32_t* ratio_up /*[n_ratios]*/, const int32_t* ratio_down /*[n_ratios]*/, int zeros,
                                      double rolloff, int n_bands /* 0: no band gains */, const double* edge_hz /*[n_bands+1]*/,
                                      const double* band_gain /*[n_terms][n_bands]*/, int64_t n_items,
                                      const int64_t* term_offset /*[n_items+1]*/, const int64_t* file /*[n_terms]*/,
                                      const int64_t* start /*[n_terms]*/, const double* gain /*[n_terms]*/,
                                      const int32_t* ratio_of /*[n_terms]: index into the list*/,
                                      const int32_t* ir_of /*[n_terms]: -1 or index into the bank*/,
                                      const int64_t* span_first /*[n_terms]*/, const int64_t* span_len /*[n_terms]*/,
                                      const int64_t* fade_in /*[n_terms] or NULL: 0*/, const int64_t* fade_out /*[n_terms] or NULL: 0*/,
                                      int64_t window, int n_channels_out, int format,
                                      void* out /* DEVICE [n_items][n_channels_out][window] */, void* stream);
int mrc_pac_store_stft_window_spans(mrc_pac_store* s, int rate_divisor, int mix, int n_ratios,
                                    const int32_t* ratio_up /*[n_ratios]*/, const int32_t* ratio_down /*[n_ratios]*/, int zeros,
                                    double rolloff, int n_bands /* 0: no band gains */, const double* edge_hz /*[n_bands+1]*/,
                                    const double* band_gain /*[n_terms][n_bands]*/, int64_t n_items,
                                    const int64_t* term_offset /*[n_items+1]*/, const int64_t* file /*[n_terms]*/,
                                    const int64_t* start /*[n_terms]*/, const double* gain /*[n_terms]*/,
                                    const int32_t* ratio_of /*[n_terms]: index into the list*/,
                                    const int32_t* ir_of /*[n_terms]: -1 or index into the bank*/,
                                    const int64_t* span_first /*[n_terms]*/, const int64_t* span_len /*[n_terms]*/,
                                    const int64_t* fade_in /*[n_terms] or NULL: 0*/, const int64_t* fade_out /*[n_terms] or NULL: 0*/,
                                    int n_fft, const double* frame_window /* HOST [n_fft] */, int64_t n_frames, int64_t hop, int mode,
                                    int n_filters, const double* bank /* HOST [n_filters][n_fft/2+1], MRC_STFT_BANK only */,
                                    int n_channels_out, int format /* MRC_WINDOW_F32 | MRC_WINDOW_F64 */, void* out /* DEVICE */,
                                    void* stream);

/* Per-stage device time of the most recent timed call when timing is enabled (hipEvents on the launch stream; the call
 * then synchronises).  Timed: mrc_dev_encode / mrc_dev_encode_ex and mrc_encode_mono / mrc_encode_joint (the _blocks
 * forms: their last shape group).  Not timed: the stage calls (mrc_dev_mdct, mrc_dev_smr, mrc_dev_alloc_quant),
 * mrc_encode_stream_pcm16* (it overlaps calls; timing stays on after it) and the chained calls (mrc_get_chain_ms).
 * ms[0..2] = mdct, smr, alloc+quant. */
int mrc_set_timing(mrc_handle* h, int enabled);
/* Options.  MRC_OPT_EXACT_SPREAD = 1: evaluate the masker spreading (psychoac.py:68-78) with the
 * reference's own expression and pow() per (masker, line) instead of the factored fast form (default 0).
 * Both give the same integer outputs on the parity corpora; the exact form is ~8x slower. */
#define MRC_OPT_EXACT_SPREAD 1
/* MRC_OPT_SMR_ALL_BANDS = 1: in joint blocks compute the SMRs of all four signals in every band (default 0: only the
 * pair the M/S switch selects per band, ms_stereo.py:70-81 -- the other pair never reaches the bit allocation). */
#define MRC_OPT_SMR_ALL_BANDS 2
/* MRC_OPT_CHAIN_FORCE_REPAIR = 1 (tests only): the chained encode's event preparation scrambles its candidate order so
 * that the repair pass, which otherwise only runs on near-ties that rounding turned round, does real work. */
#define MRC_OPT_CHAIN_FORCE_REPAIR 3
/* MRC_OPT_CHAIN_THREADS = 0 | 256 | 512 | 1024: threads of the workgroup that walks one stream in the chained encode's
 * serial scan (default 0: 512 for up to 512 streams -- the latency of the one stream counts -- else 256: eight streams per CU). */
#define MRC_OPT_CHAIN_THREADS 4
/* MRC_OPT_SENSITIVITY = 1: every encode call on the handle (not the stage calls) also counts the integer decisions it took within a guard band of
 * floating-point rounding (see mrc_get_sensitivity); costs a pass over the intermediate results (~10 % of an encode).
 * = 2 (tests): the same with every guard band 10^8 times wider, so that an ordinary corpus produces counts.
 * mrc_get_option returns the value as set (0, 1 or 2). */
#define MRC_OPT_SENSITIVITY 5
/* MRC_OPT_CHAIN_SLAB_BLOCKS = n: the chained encode (mrc_encode_chained_stream*_pac, mrc_dev_encode_chained_pac) cuts a call
 * into slabs of at most n blocks -- whole streams while they fit, a longer stream alone in consecutive time slabs, the bit
 * reservoir carried from slab to slab -- so that the device memory of a call is bounded by the slab (~45 KB per joint long
 * block + the slab's worst-case output, 13 KB per block) whatever the length of the file.  Default 131 072 (~7.5 GB; a
 * slab costs ~0.25 ms of host work between its neighbours: 8 192 streams x 12 blocks run 5 % slower in two slabs than in
 * one); 65 536: < 4 GB; 0: one slab.  The bytes do not depend on it. */
#define MRC_OPT_CHAIN_SLAB_BLOCKS 6
/* MRC_OPT_STORE_SLAB_SAMPLES = n: mrc_pac_store_decode_window cuts a call into slabs, runs of whole items whose windows sum
 * to at most n samples per channel (an item larger than n runs alone), so that its device memory is bounded by the slab
 * whatever the size of the call: 16 bytes per sample of margin planes and about as much of parsed chunks for stereo.
 * Default 2^24 (~270 MB of planes); 0: one slab.  The results do not depend on it. */
#define MRC_OPT_STORE_SLAB_SAMPLES 7
/* MRC_OPT_STORE_ROUTE_GROUP = 0 | 1 | 2: the output channels one workgroup of reverb_route_fold_kernel serves
 * (mrc_pac_store_decode_window_routed); the two channels of a group that share a source load its spectra once.  Default 0:
 * chosen per slab -- 2 where at least half of the slab's wet routes have such a neighbour (the microphones of an array), else
 * 1 (measured: DESIGN.md).  The results do not depend on it. */
#define MRC_OPT_STORE_ROUTE_GROUP 8
int mrc_set_option(mrc_handle* h, int option, int value);
int mrc_get_option(mrc_handle* h, int option, int32_t* value);
int mrc_get_stage_ms(mrc_handle* h, double* ms /*[3]*/);
/* ... and per kernel: ms[0..4] = MDCT, smr_kernel, band_stats_kernel (joint only, else ~0), bitalloc_kernel,
 * quantize_kernel.  Long blocks (1024 lines, 25 bands, 16-byte aligned planes) run the last two as one kernel,
 * alloc_quant_long_kernel: ms[3] is then the gap between two event records (a few microseconds, no kernel) and ms[4] the
 * fused kernel's time. */
int mrc_get_kernel_ms(mrc_handle* h, double* ms /*[5]*/);

#ifdef __cplusplus
}
#endif
#endif /* MRC_HIP_H */
