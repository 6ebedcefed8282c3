// Cross-lane primitives of the gfx950 kernels, each defined once (included through mrc_device.hpp): the one-wave LDS
// fence, DPP moves, the row swaps, reductions, the prefix scan and the register folds.  Everything stays in registers
// (no ds_bpermute: the LDS pipe is busy enough) and needs all 64 lanes active.  Within a 16-lane row: DPP quad
// permutes, half mirror, rotate by 8.  Across rows: gfx950's v_permlane16_swap / v_permlane32_swap exchange the odd rows
// (upper half) of one register with the even rows (lower half) of another.
#pragma once
#include <hip/hip_runtime.h>

namespace mrc {
namespace dev {

// LDS traffic between the lanes of ONE wave: order the wave's own DS operations and keep the compiler from moving LDS
// accesses across this point.  No other wave is involved.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// lane i reads the lane that DPP control CTRL names.  Every lane must have a valid source (true of the quad permutes,
// mirrors and rotates; of a row shift only for the lanes whose value is used), so no "old" value has to be prepared.
template <int CTRL>
__device__ __forceinline__ int dpp_move(int v) { return __builtin_amdgcn_mov_dpp(v, CTRL, 0xf, 0xf, true); }
template <int CTRL>
__device__ __forceinline__ unsigned dpp_move(unsigned v) { return (unsigned)dpp_move<CTRL>((int)v); }
template <int CTRL>
__device__ __forceinline__ double dpp_move(double v) {
    const int lo = dpp_move<CTRL>(__double2loint(v));
    const int hi = dpp_move<CTRL>(__double2hiint(v));
    return __hiloint2double(hi, lo);
}

// One step of a transposing butterfly at distance 16 (rows) or 32 (halves): afterwards *x holds both registers' even
// rows / lower half (a's where they were, b's in the odd rows / upper half), *y both registers' odd rows / upper half.
// Swapping a value with itself leaves {even, even} and {odd, odd} copies to combine.
typedef unsigned int uint2v __attribute__((ext_vector_type(2)));
template <int DIST>
__device__ __forceinline__ void rows_swap(unsigned a, unsigned b, unsigned* x, unsigned* y) {
    static_assert(DIST == 32 || DIST == 16, "swap distance");
    const uint2v r = DIST == 32 ? __builtin_amdgcn_permlane32_swap(a, b, false, false)
                                : __builtin_amdgcn_permlane16_swap(a, b, false, false);
    *x = r.x; *y = r.y;
}
template <int DIST>
__device__ __forceinline__ void rows_swap(int a, int b, int* x, int* y) {
    unsigned ux, uy;
    rows_swap<DIST>((unsigned)a, (unsigned)b, &ux, &uy);
    *x = (int)ux; *y = (int)uy;
}
template <int DIST>
__device__ __forceinline__ void rows_swap(double a, double b, double* x, double* y) {
    unsigned lx, ly, hx, hy;
    rows_swap<DIST>((unsigned)__double2loint(a), (unsigned)__double2loint(b), &lx, &ly);
    rows_swap<DIST>((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), &hx, &hy);
    *x = __hiloint2double((int)hx, (int)lx);
    *y = __hiloint2double((int)hy, (int)ly);
}
// op over the value at distance DIST and one's own
template <int DIST, class T, class Op>
__device__ __forceinline__ T rows_combine(T v, Op op) {
    T x, y;
    rows_swap<DIST>(v, v, &x, &y);
    return op(x, y);
}

// op over each 16-lane row, in every lane of the row
template <class T, class Op>
__device__ __forceinline__ T row_reduce(T v, Op op) {
    v = op(v, dpp_move<0xB1>(v));                       // quad_perm [1,0,3,2]
    v = op(v, dpp_move<0x4E>(v));                       // quad_perm [2,3,0,1]
    v = op(v, dpp_move<0x141>(v));                      // row_half_mirror: the other quad of the 8-lane group
    return op(v, dpp_move<0x128>(v));                   // row_ror:8: the other half of the row
}
// op over the 64 lanes, in every lane (double, int, unsigned)
template <class T, class Op>
__device__ __forceinline__ T wave_allreduce(T v, Op op) {
    v = row_reduce(v, op);
    v = rows_combine<16>(v, op);
    return rows_combine<32>(v, op);
}
__device__ __forceinline__ double wave_max(double v) {
    return wave_allreduce(v, [](double a, double b) { return fmax(a, b); });
}
__device__ __forceinline__ double wave_sum(double v) {
    return wave_allreduce(v, [](double a, double b) { return a + b; });
}
__device__ __forceinline__ int wave_sum_i(int v) {
    return wave_allreduce(v, [](int a, int b) { return a + b; });
}
__device__ __forceinline__ int wave_max_i(int v) {
    return wave_allreduce(v, [](int a, int b) { return max(a, b); });
}
// v_max_f64 as it is: fmax() makes the compiler canonicalise operands that come out of a lane exchange (a second
// v_max_f64 x, x per operand, against signalling NaNs); the values reduced with this are ratios and magnitudes
__device__ __forceinline__ double max_raw(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// maximum over each 16-lane row, in every lane of the row
__device__ __forceinline__ double row_max(double v) {
    return row_reduce(v, [](double a, double b) { return max_raw(a, b); });
}

// Four per-lane partial results -> every lane of row r (lanes 16 r .. 16 r + 15) ends with op over the whole wave's value
// r: two rounds of swaps fold the four registers into one whose rows belong to the four values, then one reduction inside
// the rows -- a quarter of four separate wave reductions.
template <class T, class Op>
__device__ __forceinline__ T wave_fold4(T a, T b, T c, T d, Op op) {
    T x, y;
    rows_swap<32>(a, c, &x, &y);                        // x = {a lower half, c lower half}, y = {a upper, c upper}
    const T ac = op(x, y);                              // lanes 0-31: value a over both halves; lanes 32-63: value c
    rows_swap<32>(b, d, &x, &y);
    const T bd = op(x, y);
    rows_swap<16>(ac, bd, &x, &y);                      // x = {ac row 0, bd row 0, ac row 2, bd row 2}, y = the odd rows
    return row_reduce(op(x, y), op);                    // row r: value r
}
// ... two values: lanes 0-31 end with op over the wave's a, lanes 32-63 with op over its b
template <class T, class Op>
__device__ __forceinline__ T wave_fold2(T a, T b, Op op) {
    T x, y;
    rows_swap<32>(a, b, &x, &y);
    return rows_combine<16>(row_reduce(op(x, y), op), op);
}

// inclusive prefix sum over the 64 lanes, in registers: Kogge-Stone inside each 16-lane row with DPP row shifts (lanes
// that would read across the row's start get 0), then the row totals are passed on with row_bcast:15 / row_bcast:31
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_shift_or_zero(int v) {
    // all rows enabled: bound_ctrl supplies the zero of lanes without a source; a partial row mask leaves the other
    // rows' lanes to the prepared zero
    if (ROW_MASK == 0xf) return __builtin_amdgcn_mov_dpp(v, CTRL, 0xf, 0xf, true);
    return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, false);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_shift_or_zero(double v) {
    return __hiloint2double(dpp_shift_or_zero<CTRL, ROW_MASK>(__double2hiint(v)),
                            dpp_shift_or_zero<CTRL, ROW_MASK>(__double2loint(v)));
}
template <class T>                                      // int or double
__device__ __forceinline__ T wave_incl_scan(T v) {
    v += dpp_shift_or_zero<0x111, 0xf>(v);              // row_shr:1
    v += dpp_shift_or_zero<0x112, 0xf>(v);              // row_shr:2
    v += dpp_shift_or_zero<0x114, 0xf>(v);              // row_shr:4
    v += dpp_shift_or_zero<0x118, 0xf>(v);              // row_shr:8
    v += dpp_shift_or_zero<0x142, 0xa>(v);              // row_bcast:15 into rows 1 and 3
    v += dpp_shift_or_zero<0x143, 0xc>(v);              // row_bcast:31 into rows 2 and 3
    return v;
}

}  // namespace dev
}  // namespace mrc
