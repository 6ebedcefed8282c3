// Probes of the __device__ helpers (mrc_wave.hpp, mrc_smr_math.hpp, the top of mrc_device.hpp): one small kernel per helper
// family that calls the helper UNCHANGED on the caller's inputs and hands the raw results back (mrc_dev_helper_probe,
// tests/test_gpu_helper_probes.py).  No helper is restated here.
//
// Transport: every array is of 8-byte words.  Word k of element j of an array with n elements sits at [k * n + j]; doubles
// travel as their bits, signed integers as int64, unsigned 32-bit values zero-extended.
//
// Every probe computes with every lane (the cross-lane primitives need all 64 active): a workgroup is 64, 128 or 256 threads,
// the grid covers n with whole workgroups, a thread past the end loads the LAST element (n >= 1) and only its store is
// guarded.  Nothing returns before a cross-lane operation.  The LDS tables are staged as the masking kernels stage them:
// 2^(j/64) (kExp2Tab), the long block's 2^(j/256) (kExp2Tab256) and the log10 table as kLogTabDev lays it out.
#include "mrc_smr_sweep.hpp"

namespace mrc {
using namespace dev;
namespace {

typedef unsigned long long u64;

// words per element of the three inputs and of the output; whether the LDS tables are staged.  wout == 0: no such probe.
struct ProbeShape { int w0, w1, w2, wout; bool tables; };
constexpr int kProbeMaxWords = 17;
constexpr ProbeShape probe_shape(int p) {
    switch (p) {
    case MRC_PROBE_MOVES_I32: case MRC_PROBE_MOVES_U32: case MRC_PROBE_MOVES_F64: return {1, 1, 0, 8, false};
    case MRC_PROBE_SUM_F64: return {1, 0, 0, 2, false};
    case MRC_PROBE_MAX_F64: return {1, 0, 0, 1, false};
    case MRC_PROBE_ROW_MAX: return {1, 0, 0, 1, false};
    case MRC_PROBE_REDUCE_I32: return {1, 0, 0, 4, false};
    case MRC_PROBE_FOLD4_F64: case MRC_PROBE_FOLD4_U32: return {4, 0, 0, 1, false};
    case MRC_PROBE_FOLD2: return {2, 2, 0, 2, false};
    case MRC_PROBE_SUM_BLOCK8: return {8, 0, 0, 8, false};
    case MRC_PROBE_SUM_ALL9: return {9, 0, 0, 9, false};
    case MRC_PROBE_SUM_ALL16: return {16, 0, 0, 16, false};
    case MRC_PROBE_SUM_ALL17: return {17, 0, 0, 17, false};
    case MRC_PROBE_SCAN_I32: case MRC_PROBE_SCAN_F64: return {1, 0, 0, 1, false};
    case MRC_PROBE_ORDER_KEY: return {1, 0, 0, 2, false};
    case MRC_PROBE_XCD: return {1, 1, 0, 1, false};
    case MRC_PROBE_RCP: return {1, 0, 0, 2, false};
    case MRC_PROBE_LINE_RATIO: return {1, 1, 0, 1, false};
    case MRC_PROBE_EXP2_POLY: return {1, 0, 0, 1, false};
    case MRC_PROBE_EXP2_TAB: return {1, 1, 0, 4, true};
    case MRC_PROBE_TABLES: return {0, 0, 0, 4, true};
    case MRC_PROBE_EXP2_DD: return {1, 1, 0, 1, false};
    case MRC_PROBE_DD_ADD: return {2, 2, 0, 2, false};
    case MRC_PROBE_ATAN_POS: return {1, 0, 0, 1, false};
    case MRC_PROBE_SPL: return {1, 1, 0, 5, true};
    case MRC_PROBE_MAG_CODE: return {1, 1, 0, 2, false};
    case MRC_PROBE_SCALE_MANT: return {1, 1, 0, 4, false};
    default: return {0, 0, 0, 0, false};
    }
}

__device__ __forceinline__ double as_f64(u64 w) { return __longlong_as_double((long long)w); }
__device__ __forceinline__ u64 bits_of(double v) { return (u64)__double_as_longlong(v); }
__device__ __forceinline__ int as_i32(u64 w) { return (int)(long long)w; }
__device__ __forceinline__ unsigned as_u32(u64 w) { return (unsigned)w; }
__device__ __forceinline__ u64 word_of(int v) { return (u64)(long long)v; }
__device__ __forceinline__ u64 word_of(unsigned v) { return (u64)v; }
__device__ __forceinline__ u64 word_of(long long v) { return (u64)v; }
__device__ __forceinline__ u64 word_of(double v) { return bits_of(v); }
template <class T> __device__ __forceinline__ T value_of(u64 w);
template <> __device__ __forceinline__ int value_of<int>(u64 w) { return as_i32(w); }
template <> __device__ __forceinline__ unsigned value_of<unsigned>(u64 w) { return as_u32(w); }
template <> __device__ __forceinline__ double value_of<double>(u64 w) { return as_f64(w); }

// the four DPP controls in use and both row swaps of (a, b)
template <class T>
__device__ __forceinline__ void probe_moves(u64 wa, u64 wb, u64* r) {
    const T a = value_of<T>(wa), b = value_of<T>(wb);
    T x, y;
    r[0] = word_of(dpp_move<0xB1>(a));
    r[1] = word_of(dpp_move<0x4E>(a));
    r[2] = word_of(dpp_move<0x141>(a));
    r[3] = word_of(dpp_move<0x128>(a));
    rows_swap<16>(a, b, &x, &y);
    r[4] = word_of(x); r[5] = word_of(y);
    rows_swap<32>(a, b, &x, &y);
    r[6] = word_of(x); r[7] = word_of(y);
}

template <int N>
__device__ __forceinline__ void probe_sum_all(const u64* a, u64* r, int lane) {
    double v[N];
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = as_f64(a[k]);
    wave_sum_all<N>(v, lane);
#pragma unroll
    for (int k = 0; k < N; ++k) r[k] = bits_of(v[k]);
}

template <int P>
__global__ __launch_bounds__(256) void probe_kernel(const u64* __restrict__ in0, const u64* __restrict__ in1,
                                                    const u64* __restrict__ in2, u64* __restrict__ out, int n) {
    constexpr ProbeShape S = probe_shape(P);
    static_assert(S.wout > 0 && S.wout <= kProbeMaxWords && S.w0 <= kProbeMaxWords, "probe shape");
    __shared__ double e2tab[kExpTab], e2long[kExpTabLong], logTab[kLogTabEntries * 4];
    if constexpr (S.tables) {
        for (int t = threadIdx.x; t < kExpTabLong; t += blockDim.x) {
            if (t < kExpTab) e2tab[t] = kExp2Tab[t];
            if (t < kLogTabEntries * 4) logTab[t] = kLogTabDev.v[t];
            e2long[t] = kExp2Tab256[t];
        }
        __syncthreads();
    }
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = i < n ? i : n - 1;                    // every lane computes; a lane past the end on the last element
    const int lane = threadIdx.x & (kWave - 1);
    u64 a[S.w0 ? S.w0 : 1] = {}, b[S.w1 ? S.w1 : 1] = {}, c[S.w2 ? S.w2 : 1] = {}, r[S.wout];
#pragma unroll
    for (int k = 0; k < S.w0; ++k) a[k] = in0[(int64_t)k * n + j];
#pragma unroll
    for (int k = 0; k < S.w1; ++k) b[k] = in1[(int64_t)k * n + j];
#pragma unroll
    for (int k = 0; k < S.w2; ++k) c[k] = in2[(int64_t)k * n + j];
    (void)c; (void)lane;

    if constexpr (P == MRC_PROBE_MOVES_I32) probe_moves<int>(a[0], b[0], r);
    else if constexpr (P == MRC_PROBE_MOVES_U32) probe_moves<unsigned>(a[0], b[0], r);
    else if constexpr (P == MRC_PROBE_MOVES_F64) probe_moves<double>(a[0], b[0], r);
    else if constexpr (P == MRC_PROBE_SUM_F64) {
        r[0] = bits_of(wave_sum(as_f64(a[0])));
        r[1] = bits_of(row_reduce(as_f64(a[0]), [](double x, double y) { return x + y; }));
    } else if constexpr (P == MRC_PROBE_MAX_F64) r[0] = bits_of(wave_max(as_f64(a[0])));
    else if constexpr (P == MRC_PROBE_ROW_MAX) r[0] = bits_of(row_max(as_f64(a[0])));
    else if constexpr (P == MRC_PROBE_REDUCE_I32) {
        const int v = as_i32(a[0]);
        r[0] = word_of(wave_sum_i(v));
        r[1] = word_of(wave_max_i(v));
        r[2] = word_of(row_reduce(v, [](int x, int y) { return x + y; }));
        r[3] = word_of(row_reduce(v, [](int x, int y) { return max(x, y); }));
    } else if constexpr (P == MRC_PROBE_FOLD4_F64) {
        r[0] = bits_of(wave_fold4(as_f64(a[0]), as_f64(a[1]), as_f64(a[2]), as_f64(a[3]),
                                  [](double x, double y) { return fmax(x, y); }));
    } else if constexpr (P == MRC_PROBE_FOLD4_U32) {
        r[0] = word_of(wave_fold4(as_u32(a[0]), as_u32(a[1]), as_u32(a[2]), as_u32(a[3]),
                                  [](unsigned x, unsigned y) { return x + y; }));
    } else if constexpr (P == MRC_PROBE_FOLD2) {
        r[0] = word_of(wave_fold2(as_i32(a[0]), as_i32(a[1]), [](int x, int y) { return x + y; }));
        r[1] = bits_of(wave_fold2(as_f64(b[0]), as_f64(b[1]), [](double x, double y) { return x + y; }));
    } else if constexpr (P == MRC_PROBE_SUM_BLOCK8) {
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = as_f64(a[k]);
        wave_sum_block<8>(v, lane);
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = bits_of(v[k]);
    } else if constexpr (P == MRC_PROBE_SUM_ALL9) probe_sum_all<9>(a, r, lane);
    else if constexpr (P == MRC_PROBE_SUM_ALL16) probe_sum_all<16>(a, r, lane);
    else if constexpr (P == MRC_PROBE_SUM_ALL17) probe_sum_all<17>(a, r, lane);
    else if constexpr (P == MRC_PROBE_SCAN_I32) r[0] = word_of(wave_incl_scan(as_i32(a[0])));
    else if constexpr (P == MRC_PROBE_SCAN_F64) r[0] = bits_of(wave_incl_scan(as_f64(a[0])));
    else if constexpr (P == MRC_PROBE_ORDER_KEY) {
        r[0] = order_key(as_f64(a[0]));
        r[1] = bits_of(order_value(r[0]));
    } else if constexpr (P == MRC_PROBE_XCD) r[0] = word_of(xcd_contiguous(as_u32(a[0]), as_u32(b[0])));
    else if constexpr (P == MRC_PROBE_RCP) {
        r[0] = bits_of(__builtin_amdgcn_rcp(as_f64(a[0])));
        r[1] = bits_of(recip_nr(as_f64(a[0])));
    } else if constexpr (P == MRC_PROBE_LINE_RATIO) r[0] = bits_of(line_ratio(as_f64(a[0]), as_f64(b[0])));
    else if constexpr (P == MRC_PROBE_EXP2_POLY) r[0] = bits_of(exp2_poly(as_f64(a[0])));
    else if constexpr (P == MRC_PROBE_EXP2_TAB) {
        const double sT = as_f64(a[0]), u = as_f64(b[0]);
        r[0] = bits_of(exp2_tab64<kExpTab>(sT, u, e2tab));
        r[1] = bits_of(exp2_tab64<kExpTabLong>(sT, u, e2long));
        r[2] = bits_of(exp2_tab_above<kExpTab>(sT, u, e2tab));
        r[3] = bits_of(exp2_tab_above<kExpTabLong>(sT, u, e2long));
    } else if constexpr (P == MRC_PROBE_TABLES) {
        r[0] = bits_of(e2tab[j & (kExpTab - 1)]);
        r[1] = bits_of(e2long[j & (kExpTabLong - 1)]);
        r[2] = bits_of(kAtanQ[j % 22]);
        r[3] = bits_of(logTab[j & (kLogTabEntries * 4 - 1)]);
    } else if constexpr (P == MRC_PROBE_EXP2_DD) r[0] = bits_of(exp2_dd(as_f64(a[0]), as_f64(b[0])));
    else if constexpr (P == MRC_PROBE_DD_ADD) {
        double hi = as_f64(a[0]), lo = as_f64(a[1]);
        dd_add(&hi, &lo, as_f64(b[0]), as_f64(b[1]));
        r[0] = bits_of(hi); r[1] = bits_of(lo);
    } else if constexpr (P == MRC_PROBE_ATAN_POS) r[0] = bits_of(atan_pos(as_f64(a[0])));
    else if constexpr (P == MRC_PROBE_SPL) {
        const double x = as_f64(a[0]);
        r[0] = bits_of(spl_db_tab(x, logTab));
        r[1] = bits_of(spl_db(x));
        r[2] = bits_of(log10_tab32(x, logTab));         // (reads table entry (bits >> 47) & 31 whatever x is)
        double thr;
        r[3] = bits_of(excess_plain(x, as_f64(b[0]), 3, logTab, &thr));
        r[4] = bits_of(thr);
    } else if constexpr (P == MRC_PROBE_MAG_CODE) {
        const int nBits = min(max(as_i32(b[0]), 1), 31);                   // the widths the unsigned code holds
        r[0] = word_of(mag_code<unsigned>(as_f64(a[0]), nBits));
        r[1] = word_of(mag_code<long long>(as_f64(a[0]), nBits));
    } else if constexpr (P == MRC_PROBE_SCALE_MANT) {
        // settings word: scale | nScaleBits << 8 | nMantBits << 16, clamped to what the encoder's widths allow
        const int w = as_i32(b[0]);
        const int nScaleBits = min(max((w >> 8) & 0xff, 1), 4), nMantBits = min(max((w >> 16) & 0xff, 2), 16);
        const int scale = min(w & 0xff, (1 << nScaleBits) - 1);
        const double x = as_f64(a[0]);
        r[0] = word_of(scale_factor_dev<unsigned>(x, nScaleBits, nMantBits));
        r[1] = word_of(scale_factor_dev<long long>(x, nScaleBits, nMantBits));
        r[2] = word_of(mantissa_dev<unsigned>(x, scale, nScaleBits, nMantBits));
        r[3] = word_of(mantissa_dev<long long>(x, scale, nScaleBits, nMantBits));
    }

    if (i < n) {
#pragma unroll
        for (int k = 0; k < S.wout; ++k) out[(int64_t)k * n + i] = r[k];
    }
}

template <int P>
hipError_t launch_one(const void* in0, const void* in1, const void* in2, void* out, int n, int threads, hipStream_t st) {
    hipLaunchKernelGGL(probe_kernel<P>, dim3((unsigned)((n + threads - 1) / threads)), dim3(threads), 0, st, (const u64*)in0,
                       (const u64*)in1, (const u64*)in2, (u64*)out, n);
    return hipGetLastError();
}

}  // namespace

bool probe_words(int probe, int* w0, int* w1, int* w2, int* wout) {
    const ProbeShape S = probe_shape(probe);
    *w0 = S.w0; *w1 = S.w1; *w2 = S.w2; *wout = S.wout;
    return S.wout > 0;
}

hipError_t launch_probe(int probe, const void* in0, const void* in1, const void* in2, void* out, int n, int threads,
                        hipStream_t st) {
    switch (probe) {
#define MRC_PROBE_CASE(P) case P: return launch_one<P>(in0, in1, in2, out, n, threads, st);
    MRC_PROBE_CASE(MRC_PROBE_MOVES_I32) MRC_PROBE_CASE(MRC_PROBE_MOVES_U32) MRC_PROBE_CASE(MRC_PROBE_MOVES_F64)
    MRC_PROBE_CASE(MRC_PROBE_SUM_F64) MRC_PROBE_CASE(MRC_PROBE_MAX_F64) MRC_PROBE_CASE(MRC_PROBE_ROW_MAX)
    MRC_PROBE_CASE(MRC_PROBE_REDUCE_I32) MRC_PROBE_CASE(MRC_PROBE_FOLD4_F64) MRC_PROBE_CASE(MRC_PROBE_FOLD4_U32)
    MRC_PROBE_CASE(MRC_PROBE_FOLD2) MRC_PROBE_CASE(MRC_PROBE_SUM_BLOCK8) MRC_PROBE_CASE(MRC_PROBE_SUM_ALL9)
    MRC_PROBE_CASE(MRC_PROBE_SUM_ALL16) MRC_PROBE_CASE(MRC_PROBE_SUM_ALL17) MRC_PROBE_CASE(MRC_PROBE_SCAN_I32)
    MRC_PROBE_CASE(MRC_PROBE_SCAN_F64) MRC_PROBE_CASE(MRC_PROBE_ORDER_KEY) MRC_PROBE_CASE(MRC_PROBE_XCD)
    MRC_PROBE_CASE(MRC_PROBE_RCP) MRC_PROBE_CASE(MRC_PROBE_LINE_RATIO) MRC_PROBE_CASE(MRC_PROBE_EXP2_POLY)
    MRC_PROBE_CASE(MRC_PROBE_EXP2_TAB) MRC_PROBE_CASE(MRC_PROBE_TABLES) MRC_PROBE_CASE(MRC_PROBE_EXP2_DD)
    MRC_PROBE_CASE(MRC_PROBE_DD_ADD) MRC_PROBE_CASE(MRC_PROBE_ATAN_POS) MRC_PROBE_CASE(MRC_PROBE_SPL)
    MRC_PROBE_CASE(MRC_PROBE_MAG_CODE) MRC_PROBE_CASE(MRC_PROBE_SCALE_MANT)
#undef MRC_PROBE_CASE
    default: return hipErrorInvalidValue;
    }
}

}  // namespace mrc
