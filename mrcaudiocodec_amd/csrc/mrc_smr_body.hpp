// smr_kernel (psychoac.py:134-219 for one (frame, signal) unit per workgroup; overview in mrc_kernels_smr.hip) for the two units
// that instantiate it: mrc_kernels_smr.hip, and mrc_kernels_smr_mono.hip for the one instantiation with its own scheduler option.
#pragma once
#include "mrc_smr_sweep.hpp"

#include <type_traits>

namespace mrc {
using namespace dev;
namespace {

constexpr int kLinesPerThread = 4;                     // EXACT mode register tile

// waves per SIMD.  Long / transition / generic blocks: 4 workgroups of 4 waves per CU (what the LDS footprint allows): <= 128 VGPRs.
// Short blocks (two waves, ~5 KB of LDS per workgroup) are latency-bound: more waves.  Measured per 114 688 short units: 4 waves
// per SIMD 0.714 ms, 5: 0.657, 6: 0.627, 8: 0.612 -- but at 8 (64 registers) 16 registers spill and the scratch traffic is
// 1 GB per step of configs[3] (PMC WRITE_SIZE); 6 (77 registers) spills none.
constexpr int kSmrWavesPerSimd = 4, kSmrWavesPerSimdShort = 6;
// issue priority (0..3) of a wave until it enters the sweep, and during the far-field pass (shuffle-heavy reductions)
constexpr int kFrontPrio = 3, kFarPrio = 0;

// DIM: 1024 = the long block (N = 2048: H = M = 1024, 924 bins searched for peaks), 128 = the short block (N = 256: H = M =
// 128, 28 bins), 576 = the transition blocks (N = 1152) with their dimensions as compile-time constants -- loop bounds, index splits and the LDS layout fold into
// immediates; same arithmetic, same results.  0: any shape, dimensions from DevShape.
// MODE: what the hot paths fix at compile time -- 1: mono (one signal per frame, every band wanted, no thresholds out, band
// peaks out); 2: joint stereo with the M/S switch known (four signals, the rest alike); 0: all of it at run time.
template <bool EXACT, class SampleT, int NT, int DIM, int MODE>
__device__ __forceinline__ void smr_body(DevShape S, int nsigArg, const SampleT* __restrict__ chL,
                                         const SampleT* __restrict__ chR, int64_t stride,
                                         const int64_t* __restrict__ offsetsArg, const double* __restrict__ lines,
                                         const int* __restrict__ oscale, double* __restrict__ smr,
                                         double* __restrict__ threshArg, double* __restrict__ bandPeakArg,
                                         const int* __restrict__ msSwitch, SmrLds layArg,
                                         unsigned long long* __restrict__ sens) {
    extern __shared__ double smem[];
    const SmrLds lay = DIM ? smr_layout(DIM, DIM, DIM - 100, nullptr) : layArg;
    __shared__ int waveCnt[NT / kWave];
    // per-band running max of the excess (order-preserving key), per-band max |X| (the bit pattern of |x| orders like |x|).
    __shared__ unsigned long long bandKey[kMaxBands], peakKey[kMaxBands];
    __shared__ unsigned long long slopeKey[2];          // min / max upper slope over the frame's maskers (keys)
    __shared__ unsigned char needBand[kMaxBands];       // joint blocks: does the encoder use THIS signal's SMR of the band?
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1), wave = tid >> 6;
    constexpr bool LONG = DIM == 1024;
    const int nsig = MODE == 1 ? 1 : MODE == 2 ? 4 : nsigArg;
    const bool haveSwitch = MODE == 1 ? false : MODE == 2 ? true : msSwitch != nullptr;
    const int64_t* offsets = offsetsArg;                 // (strided frames or explicit block offsets: one select per unit either way)
    double* thresh = MODE ? nullptr : threshArg;
    double* bandPeak = bandPeakArg;
    const bool wantPeak = MODE ? true : bandPeakArg != nullptr;
    const int H = DIM ? DIM : S.H, M = DIM ? DIM : S.halfN;
    const int last = DIM ? DIM - 100 : S.peakLast;      // bins 0 .. last-1 are inspected (psychoac.py:160)
    // XCD-aware order: workgroups are dealt round-robin to the 8 XCDs (each with its own L2), so hardware block
    // i + 1 runs on another die than block i.  Unit u below is chosen such that every XCD walks a CONTIGUOUS range of
    // (frame, signal) units: neighbouring frames share a hop, and the four signals of a joint frame share all their
    // samples -- with this order the second reader finds them in its own L2 instead of fetching them from HBM again.
    // The four signals of a joint frame cost differently (the sweep skips what the M/S switch does not use), and the
    // hardware deals consecutive workgroups to the shader engines round-robin: with sig = unit % 4 every engine would see
    // ONE signal only and the kernel would wait for the engines with the expensive ones.  Rotating the signals from frame
    // to frame gives every engine the same mix.
    const unsigned slot = xcd_contiguous(blockIdx.x, gridDim.x);
    const int64_t f = slot / nsig;
    const int sig = (int)((slot + f) % nsig);
    const unsigned unit = (unsigned)(f * nsig + sig);
    // A joint unit NONE of whose bands the M/S switch selects (all bands M/S: the L and R units; all bands L/R: the M and S
    // units -- the rule for strongly correlated and for unrelated channels) has no reader at all: neither its SMRs nor its band
    // peaks reach the bit allocation or the scale factors (ms_stereo.py:70-81; mrc_kernels_alloc.hip reads the selected
    // signal of every band only).  It ends here, before its first load; its outputs stay unwritten.  Every wave takes the
    // same decision from the same 25 flags: no barrier.
    if (haveSwitch && !thresh) {
        const bool need = lane < S.nBands && ((sig >= 2) == (msSwitch[f * S.nBands + lane] != 0));
        if (!__any(need)) return;
    }
    const int64_t off = offsets ? offsets[f] : f * stride;
    double2* A = (double2*)smem;                        // [H]
    double2* B = A + H;                                 // [H]
    double* xi = smem + 4 * H;    // [peakLast + 1] intensity spectrum; later the suffix sums
    // region B is free once the spectrum is in xi: peak bins, then per-line masker counts (filled below)
    unsigned short* cntArr = reinterpret_cast<unsigned short*>(smem + 2 * H);   // [M + 1]
    unsigned short* nUpArr = cntArr + (M + 2);                           // [M + 1]
    short* pkBin = reinterpret_cast<short*>(nUpArr + (M + 2));           // [<= peakLast/2 + 1] peak bins, increasing; dead after
                                                                         // the masker table (then the start of the node rows)
    double* piHi = reinterpret_cast<double*>(pkBin + ((last / 2 + 5) & ~3));   // [<= peakLast/2 + 2] prefix sums of
    double* piLo = piHi + (last / 2 + 2);                //   the masker intensities, double-double (hi, lo)

#ifdef MRC_PROFILE_PHASES
    __shared__ unsigned long long sPhase_[32];
    if (threadIdx.x < 32) sPhase_[threadIdx.x] = 0ull;
    __syncthreads();
    long long tPhase_ = __builtin_readcyclecounter();
#endif
    // The phases before the sweep are chains of short instruction bursts between barriers and memory waits; the sweep
    // is one long stream of VALU work.  Waves of the four workgroups that share a SIMD are in different phases: the
    // ones in the latency-bound part get issue priority, so their chain is not stretched by a neighbour's sweep.
    __builtin_amdgcn_s_setprio(kFrontPrio);
    if (tid < kMaxBands) bandKey[tid] = 0ull; // below every key; visible after the first barrier
    if (tid < 2) slopeKey[tid] = tid ? 0ull : ~0ull;
    if (tid < kMaxBands) peakKey[tid] = 0ull;
    // ms_stereo.py:70-81 (OverallSMRs) keeps, per band, either the L / R pair of SMRs or the M / S pair: the other two
    // never reach the bit allocation.  With the switch known (it only needs the MDCT lines) the sweep below leaves out
    // the 64-line chunks none of whose bands want this signal -- half of all (signal, band) pairs of a stereo frame.
    if (tid < kMaxBands)
        needBand[tid] = (!haveSwitch || tid >= S.nBands) ? 1 : (((sig >= 2) == (msSwitch[f * S.nBands + tid] != 0)) ? 1 : 0);
    const double* zbS = smem + lay.zbOff;               // staged after the FFT (the area is FFT scratch / dead)
    // 2^(j/T): T = 64 in the tail of region A, behind the masker table; the long block's sweep: T = 256, in the half of the
    // spectrum area the suffix sums leave free (staged when the spectrum is dead, with the scans)
    constexpr int TAB = (DIM == 1024 && !EXACT && NT == 256) ? kExpTabLong : kExpTab;
    constexpr int kTabLongOff = 464;                    // (doubles behind the start of the spectrum area; sc takes <= 462)
    const double* e2tab = TAB == kExpTab ? smem + 2 * H - kExpTab : smem + 4 * H + kTabLongOff;
    // per-band max of (line intensity / masked threshold) as the bit pattern of a positive double; in front of e2tab
    unsigned long long* ratioKey = reinterpret_cast<unsigned long long*>(smem + 2 * H - kExpTab - kMaxBands);
    const double* logTabLds = smem + lay.logOff;
    const double* logTab = logTabLds;
    // Hann window (window.py:28-45) and real FFT through an H = N/2 point complex FFT.  The raw words of a thread's
    // kPre sample pairs and their Hann values are all requested before the first of them is converted (`front` below;
    // the long block is one such group): one memory round trip per group instead of one per pair.
    constexpr int kPre = 4;
    // (even, odd) sample pairs come as ONE load each when the block starts at an even sample of an aligned channel
    const bool pairAligned = !(off & 1) && !(reinterpret_cast<uintptr_t>(chL) & (2 * sizeof(SampleT) - 1)) &&
                             (!chR || !(reinterpret_cast<uintptr_t>(chR) & (2 * sizeof(SampleT) - 1)));
    // long blocks: a thread's four samples are the inputs of its first butterfly and stay in registers (fft_regs_1024)
    MRC_PHASE(16);
    constexpr bool kFftRegs = LONG && NT == 256 && kPre == 4;
    constexpr bool kSplitPairs = kFftRegs;                 // ... and the real split takes bins k and H - k together
    [[maybe_unused]] double2 fftIn[4];
    [[maybe_unused]] Tw3 fftW1;
    if constexpr (kFftRegs) fftW1 = fft1024_twiddles(S.fftTw, 1, tid);
    // One arm per (alignment, signal kind), chosen once per unit (both are wave-uniform): decided per pair, each pair's
    // load ended up in a basic block of its own with a full wait behind it -- four dependent round trips for int16 PCM.
    // MS: the M / S signals, which read both channels; else the one channel of L or R.
    auto front = [&](auto alignedC, auto msC) {
        constexpr bool AL = decltype(alignedC)::value, MS = decltype(msC)::value;
        const SampleT* const one = MS ? chL : (sig == 1 ? chR : chL);
        for (int n0 = tid; n0 < H; n0 += NT * kPre) {
            decltype(raw_pair<AL>(one, 0)) rawL[kPre];
            [[maybe_unused]] decltype(raw_pair<AL>(one, 0)) rawR[kPre];
            double2 hn[kPre];
#pragma unroll
            for (int u = 0; u < kPre; ++u) {
                const int n = min(n0 + u * NT, H - 1);
                rawL[u] = raw_pair<AL>(one, off + 2 * n);
                if constexpr (MS) rawR[u] = raw_pair<AL>(chR, off + 2 * n);
                hn[u] = make_double2(S.hann[2 * n], S.hann[2 * n + 1]);
            }
#pragma unroll
            for (int u = 0; u < kPre; ++u) {
                const int n = n0 + u * NT;
                double2 eo = pair_value(rawL[u]);
                if constexpr (MS) {                      // codecThem.py:363-364
                    const double2 r = pair_value(rawR[u]);
                    eo = sig == 2 ? make_double2((eo.x + r.x) / 2.0, (eo.y + r.y) / 2.0)
                                  : make_double2((eo.x - r.x) / 2.0, (eo.y - r.y) / 2.0);
                }
                if constexpr (kFftRegs) fftIn[u] = make_double2(eo.x * hn[u].x, eo.y * hn[u].y);
                else if (n < H) A[n] = make_double2(eo.x * hn[u].x, eo.y * hn[u].y);
            }
        }
    };
    auto front_kind = [&](auto alignedC) {
        if constexpr (MODE == 1) front(alignedC, std::false_type{});
        else if (sig >= 2) front(alignedC, std::true_type{});
        else front(alignedC, std::false_type{});
    };
    if (pairAligned) front_kind(std::true_type{});
    else front_kind(std::false_type{});
    // (the unit's scale is first used in the sweep: requested here, it arrives under the wait for the samples)
    const int scale = oscale[unit];
    const double xiInv = 1.0 / S.xiDen;
    // Constants that are only needed after the FFT are requested BEFORE it (their LDS homes are FFT scratch until
    // then): the loads complete under the FFT's barriers instead of adding a memory round trip of their own.
    double2 wnPre[kPre];
    double zbPre[kPre], logPre = 0.0, e2Pre = 0.0;
    [[maybe_unused]] double e2Pre64 = 0.0;              // long blocks: the 64-entry table too (the node terms are built while
                                                        // the 256-entry one is being staged)
#pragma unroll
    for (int u = 0; u < kPre; ++u) {
        // (long blocks: the real split below works on the pairs (k, H - k), k = tid + 1, tid + 1 + NT)
        if (!kSplitPairs || u < 2) wnPre[u] = S.wN[kSplitPairs ? tid + 1 + u * NT : min(tid + u * NT, last - 1)];
        zbPre[u] = EXACT ? 0.0 : S.zb[min(tid + u * NT, M - 1)];
    }
    if (!EXACT) {
        logPre = kLogTabDev.v[tid & (kLogTabEntries * 4 - 1)];
        e2Pre = TAB == kExpTab ? kExp2Tab[tid & (kExpTab - 1)] : kExp2Tab256[tid & 255];
        if (TAB != kExpTab) e2Pre64 = kExp2Tab[tid & (kExpTab - 1)];
    }
    double2* T;
    if constexpr (kFftRegs) {
        MRC_PHASE(0); MRC_STOP(0);
        T = fft_regs_1024(fftIn, A, B, S.fftTw, fftW1, tid);
    } else if (lay.twOff >= 0) {
        double2* Wq = reinterpret_cast<double2*>(smem + lay.twOff);
        for (int t = tid; t < H / 4; t += NT) Wq[t] = S.wH[t];
        __syncthreads();
        MRC_PHASE(0); MRC_STOP(0);
        if (LONG && NT == 256) T = fft_lds_1024<NT>(A, B, Wq, tid);
        else if (DIM == 128) T = fft_lds_128<NT>(A, B, Wq, tid);
        else
        T = fft_lds_pow2<NT>(A, B, H, S.radH, S.nRadH, TwQuarter{Wq, H / 4 - 1, 31 - __clz(H / 4)}, tid);
    } else {
        __syncthreads();
        MRC_PHASE(0); MRC_STOP(0);
        if (DIM == 576) T = fft_lds_576<NT>(A, B, S.wH, tid);
        else
        T = fft_lds_global<NT>(A, B, H, S.radH, S.nRadH, S.wH, tid);
    }
    MRC_PHASE(1); MRC_STOP(1);
    if constexpr (kSplitPairs) {
        // Bins k and H - k come from the same two values of T: with Xe = (T[k] + conj T[H-k]) / 2, Xo = (T[k] - conj T[H-k]) / 2i
        // and P = w_k Xo, X[k] = Xe + P and X[H-k] = conj(Xe - P) (w_{H-k} = -conj w_k).  A thread takes two pairs -- half the
        // reads of T and one complex product for two bins; bin k exactly as below, bin H - k as below with the mirrored twiddle.
        auto intensity = [&](double2 X) {
            return EXACT ? 4. * (X.x * X.x + X.y * X.y) / S.xiDen : (4. * (X.x * X.x + X.y * X.y)) * xiInv;   // psychoac.py:151
        };
        auto split = [&](int k, double2 w, bool both) {
            const double2 zk = T[k];
            double2 zc = T[(H - k) & (H - 1)];
            zc.y = -zc.y;
            const double2 ev = make_double2(0.5 * (zk.x + zc.x), 0.5 * (zk.y + zc.y));
            const double2 d = make_double2(zk.x - zc.x, zk.y - zc.y);
            const double2 od = make_double2(0.5 * d.y, -0.5 * d.x);
            const double2 P = cmul(w, od);
            xi[k] = intensity(make_double2(P.x + ev.x, P.y + ev.y));
            if (both) xi[H - k] = intensity(make_double2(ev.x - P.x, ev.y - P.y));
        };
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int k = tid + 1 + u * NT;              // 1 .. H / 2
            split(k, wnPre[u], H - k < last && k != H / 2);
        }
        if (tid == 0) split(0, make_double2(1.0, 0.0), false);
    } else
    for (int k0 = tid; k0 < last; k0 += NT * kPre) {
        double2 wn[kPre];
#pragma unroll
        for (int u = 0; u < kPre; ++u) wn[u] = (k0 == tid) ? wnPre[u] : S.wN[min(k0 + u * NT, last - 1)];
#pragma unroll
        for (int u = 0; u < kPre; ++u) {
            const int k = k0 + u * NT;
            if (k < last) {
                double2 zk = T[k];
                double2 zc = T[(H - k) % H];
                zc.y = -zc.y;
                double2 ev = make_double2(0.5 * (zk.x + zc.x), 0.5 * (zk.y + zc.y));
                double2 d = make_double2(zk.x - zc.x, zk.y - zc.y);
                double2 od = make_double2(0.5 * d.y, -0.5 * d.x);
                double2 X = cmul(wn[u], od);
                X.x += ev.x; X.y += ev.y;
                xi[k] = EXACT ? 4. * (X.x * X.x + X.y * X.y) / S.xiDen      // psychoac.py:151
                              : (4. * (X.x * X.x + X.y * X.y)) * xiInv;     // (one rounding more)
            }
        }
    }
    MRC_PHASE(20);
    __syncthreads();                                    // T (in A or B) is dead from here on
    MRC_PHASE(2); MRC_STOP(2);
    if (!EXACT) {                                       // stage the Bark grid and the log10 table (used after 2 barriers)
        {
            double* zw = smem + lay.zbOff;
#pragma unroll
            for (int u = 0; u < kPre; ++u)
                if (tid + u * NT < M) zw[tid + u * NT] = zbPre[u];
            for (int k = tid + kPre * NT; k < M; k += NT) zw[k] = S.zb[k];
        }
        if (tid < kLogTabEntries * 4) smem[lay.logOff + tid] = logPre;
        if (tid < kExpTab) smem[2 * H - kExpTab + tid] = TAB == kExpTab ? e2Pre : e2Pre64;
        if (tid < kMaxBands) ratioKey[tid] = 0ull;
    }

    // tonal maskers: strict 3-point peaks at bins p = 1 .. last-2, kept in increasing bin order.
    // Table (aliases A), 4 doubles per masker:
    //   EXACT: {level-15 dB, Bark z, 0.37*max(level-40,0), -}
    //   fast : {I = 10^((level-15-96)/10), Bark z, upper slope in bits/Bark, I * 2^(b z)}
    double* mt = smem;
    const int nCand = last - 2;
    const int per = (nCand + NT - 1) / NT;
    const int p0 = 1 + tid * per;
    const int p1 = min(p0 + per, last - 1);
    // a thread's candidate bins and their neighbours are read ONCE (per + 2 values); the peak flags serve the count, the
    // ordered compaction behind the barrier and (MRC_OPT_SENSITIVITY) the near-tie count
    constexpr int kPerMax = 4;                           // long block: 4 candidates per thread, transition: 2, short: 1
    int mine = 0;
    unsigned flags = 0;
    if (per <= kPerMax) {
        double v[kPerMax + 2];
#pragma unroll
        for (int j = 0; j < kPerMax + 2; ++j) v[j] = xi[min(p0 - 1 + j, last - 1)];
#pragma unroll
        for (int j = 0; j < kPerMax; ++j)
            if (p0 + j < p1 && v[j + 1] > v[j] && v[j + 1] > v[j + 2]) flags |= 1u << j;
        mine = __popc(flags);
        if (sens) {
            // MRC_OPT_SENSITIVITY: strict comparisons of psychoac.py:162 that a relative change of kPeakGuard in a bin would
            // turn round (a bin within the guard of a neighbour it has to beat, while it does not clearly lose against the other)
            const double kPeakGuard = 1e-11 * __longlong_as_double((long long)sens[7]);    // (sens[7]: guard scale, 1 or 1e8)
            int near = 0;
#pragma unroll
            for (int j = 0; j < kPerMax; ++j) {
                const double c = v[j + 1], l = v[j], r = v[j + 2];
                const bool nl = fabs(c - l) <= kPeakGuard * c, nr = fabs(c - r) <= kPeakGuard * c;
                near += (p0 + j < p1 && ((nl && (c > r || nr)) || (nr && (c > l || nl)))) ? 1 : 0;
            }
            if (near) atomicAdd(&sens[3], (unsigned long long)near);
        }
    } else {
        for (int p = p0; p < p1; ++p) mine += (xi[p] > xi[p - 1] && xi[p] > xi[p + 1]) ? 1 : 0;
    }
    const int incl = wave_incl_scan(mine);
    if (lane == kWave - 1) waveCnt[wave] = incl;
    MRC_PHASE(17);
    __syncthreads();
    MRC_PHASE(18);
    int before = incl - mine, nPeaks = 0;
    for (int w = 0; w < NT / kWave; ++w) {
        const int c = waveCnt[w];
        if (w < wave) before += c;
        nPeaks += c;
    }
    // compact the peak bins first (ordered), then one masker per thread: the transcendental-heavy
    // table entry is computed by full waves instead of the few lanes that happen to own a peak
    if (per <= kPerMax) {
#pragma unroll
        for (int j = 0; j < kPerMax; ++j)
            if ((flags >> j) & 1u) pkBin[before++] = (short)(p0 + j);
    } else {
        for (int p = p0; p < p1; ++p)
            if (xi[p] > xi[p - 1] && xi[p] > xi[p + 1]) pkBin[before++] = (short)p;
    }
    if (!EXACT) {                                        // the two count histograms (adjacent: 2 (M + 2) shorts), eight bytes a store
        unsigned long long* z = reinterpret_cast<unsigned long long*>(cntArr);
        for (int k = tid; k < (M + 2) / 2; k += NT) z[k] = 0ull;
    }
    MRC_PHASE(19);
    __syncthreads();
    MRC_PHASE(3); MRC_STOP(3);
    double slLo = 1e300, slHi = -1e300;                 // this thread's maskers: range of the upper slope
    for (int mi = tid; mi < nPeaks; mi += NT) {
        const int before = mi;
        const int p = pkBin[mi];
        const double x0 = xi[p - 1], x1 = xi[p], x2 = xi[p + 1];
        {
            double s3 = (x0 + x1) + x2;
            MRC_PHASE(21);
            double level = EXACT ? spl_db(s3) : spl_db_tab(s3, logTabLds);   // psychoac.py:164
            const double fnum = S.binHz * (((p - 1) * x0 + p * x1) + (p + 1) * x2);
            double fm = EXACT ? fnum / s3 : fnum * recip_nr(s3);                  // psychoac.py:165
            // psychoac.py:27-29.  The fast path multiplies by the reciprocals of the constants 7500, 1000 and 10
            // (one rounding more each, against ~12 instructions per fp64 division) and uses atan_pos; EXACT divides and
            // calls atan like the reference
            double q = EXACT ? fm / 7500. : fm * (1. / 7500.);
            const double zm = EXACT ? 13 * atan(0.76 * fm / 1000.) + 3.5 * atan(q * q)
                                    : 13 * atan_pos((0.76 * fm) * 1e-3) + 3.5 * atan_pos(q * q);
            const double lvl15 = level - 15.0;                               // psychoac.py:42-43 (tonal drop)
            const double boost = 0.37 * fmax(level - 40, 0.0);               // psychoac.py:76
            double* e = mt + 4 * before;
            if (EXACT) {
                e[1] = zm;
                e[0] = lvl15;
                e[2] = boost;
            } else {
                // psychoac.py:14-18: 10^((spl-96)/10) as 2^(x log2 10), exponent in double-double (<= 1 ulp)
                const double xe = (lvl15 - 96) * 0.1;
                const double eh = xe * kLog2Of10;
                const double I = exp2_dd(eh, fma(xe, kLog2Of10, -eh) + xe * kLog2Of10Lo);
                const double ph = kLowHi * zm;
                const double pl = fma(kLowHi, zm, -ph) + kLowLo * zm;
                // (the entry leaves as two 16-byte stores: 8-byte stores 32 bytes apart from lane to lane meet on four banks)
                const double slope = (((-27 + boost) * 0.1) * kLog2Of10) * (double)TAB;  // upper slope, 1/T bit per Bark
                slLo = fmin(slLo, slope);
                slHi = fmax(slHi, slope);
                reinterpret_cast<double2*>(e)[0] = make_double2(I, zm);
                reinterpret_cast<double2*>(e)[1] = make_double2(slope, I * exp2_dd(ph, pl));
                // first line that sees this masker at all (fl(z_k - z_m) >= -1/2) and first line more than
                // 1/2 Bark above it (fl(z_k - z_m) > 1/2): both predicates are monotone in k
                // The searches start from the precomputed answers for the line nearest to the masker's own
                // frequency and walk to the exact boundary (a step or two; any start gives the same result).
                const int kNear = min(max((int)(fm * S.linesPerHz), 0), M - 1);
                MRC_PHASE(22);
                int lo = S.loLine[kNear], hi = S.hiLine[kNear];
#ifdef MRC_PROFILE_PHASES
                asm volatile("" : "+v"(lo), "+v"(hi));
#endif
                MRC_PHASE(23);
                // The hints are the answers for the Bark value of line kNear, less than a line away from z_m: the boundary
                // is the hinted line or a neighbour.  Both windows (hint - 2 .. hint + 1) are read at once and decided in
                // registers -- one LDS round trip instead of one per step of four dependent loops; whoever is not settled by
                // that (never, on the corpora of the tests) walks as before.
                {
                    auto zAt = [&](int k) { return zbS[min(max(k, 0), M - 1)]; };
                    const double a0 = zAt(lo - 2), a1 = zAt(lo - 1), a2 = zAt(lo), a3 = zAt(lo + 1);
                    const double b0 = zAt(hi - 2), b1 = zAt(hi - 1), b2 = zAt(hi), b3 = zAt(hi + 1);
                    // (line M stands for "no line": the predicate holds there; below line 0 it does not)
                    auto sees = [&](double zv, int k) { return k >= M || (k >= 0 && zv - zm >= -0.5); };
                    auto above = [&](double zv, int k) { return k >= M || (k >= 0 && zv - zm > 0.5); };
                    const bool s0 = sees(a0, lo - 2), s1 = sees(a1, lo - 1), s2 = sees(a2, lo), s3 = sees(a3, lo + 1);
                    const bool u0 = above(b0, hi - 2), u1 = above(b1, hi - 1), u2 = above(b2, hi), u3 = above(b3, hi + 1);
                    const int first = (s1 && !s0) ? lo - 1 : (s2 && !s1) ? lo : (s3 && !s2) ? lo + 1 : -1;
                    const int over = (u1 && !u0) ? hi - 1 : (u2 && !u1) ? hi : (u3 && !u2) ? hi + 1 : -1;
                    if (__any(first < 0 || over < 0)) {
                        while (lo > 0 && zbS[lo - 1] - zm >= -0.5) --lo;
                        while (lo < M && !(zbS[lo] - zm >= -0.5)) ++lo;
                        hi = max(hi, lo);
                        while (hi > 0 && zbS[hi - 1] - zm > 0.5) --hi;
                        while (hi < M && !(zbS[hi] - zm > 0.5)) ++hi;
                    } else {
                        lo = first;
                        hi = over;
                    }
                }
                atomicAdd(reinterpret_cast<unsigned int*>(cntArr) + (lo >> 1), 1u << (16 * (lo & 1)));
                atomicAdd(reinterpret_cast<unsigned int*>(nUpArr) + (hi >> 1), 1u << (16 * (hi & 1)));
                MRC_PHASE(24);
            }
        }
    }
    if (!EXACT) {
        slLo = -wave_max(-slLo);
        slHi = wave_max(slHi);
        if (lane == 0) {
            atomicMin(&slopeKey[0], order_key(slLo));
            atomicMax(&slopeKey[1], order_key(slHi));
        }
    }
    MRC_PHASE(4);
    __syncthreads();
    MRC_PHASE(12); MRC_STOP(4);

    // psychoac.py:214-217: SMR of a band = max over its lines of (SPL of the line - masked threshold),
    // accumulated with LDS integer max-atomics on an order-preserving key (initialised by the table
    // build's barrier below)
    const double* X = lines + (int64_t)unit * M;

    if (EXACT) {
        for (int base = 0; base < M; base += NT * kLinesPerThread) {
            double z[kLinesPerThread], tot[kLinesPerThread];
#pragma unroll
            for (int j = 0; j < kLinesPerThread; ++j) {
                int k = base + tid + j * NT;
                bool ok = k < M;
                z[j] = ok ? S.zb[k] : 0.0;
                tot[j] = ok ? S.quiet[k] : 0.0;
            }
            // psychoac.py:166-168 + 68-78: add every masker's spread intensity, in masker order
            for (int m = 0; m < nPeaks; ++m) {
                const double lvl = mt[4 * m], zm = mt[4 * m + 1], boost = mt[4 * m + 2];
#pragma unroll
                for (int j = 0; j < kLinesPerThread; ++j) {
                    double dz = z[j] - zm;
                    double adz = fabs(dz);
                    double t = adz - 0.5;
                    double arg = lvl;
                    if (adz > 0.5) arg = lvl + (-27 * t);
                    if (dz > 0.5) arg = arg + boost * t;
                    tot[j] += pow(10.0, (arg - 96) / 10);
                }
            }
#pragma unroll
            for (int j = 0; j < kLinesPerThread; ++j) {
                int k = base + tid + j * NT;
                if (k < M) {
                    double thr = spl_db(tot[j]);                                 // psychoac.py:173
                    if (thresh) thresh[(int64_t)unit * M + k] = thr;
                    double xs = ldexp(X[k], scale);                              // codecThem.py:323 (exact)
                    double spl = spl_db(2. * (xs * xs) / (1. / 2.)) - 6. * scale;   // psychoac.py:212
                    atomicMax(&bandKey[S.bandOfLine[k]], order_key(spl - thr));
                    if (wantPeak)
                        atomicMax(&peakKey[S.bandOfLine[k]], (unsigned long long)__double_as_longlong(fabs(X[k])));
                }
            }
        }
    } else {
        // suffix sums of the lower-side constants: sc[m] = sum_{j >= m} I_j 2^(b z_j), sc[nPeaks] = 0
        double* sc = xi;                                 // xi is dead (all peak reads happened before the barrier)
        if (TAB != kExpTab) smem[4 * H + kTabLongOff + tid] = e2Pre;      // (NT = 256 = TAB: an entry per thread)
        const int waveU = __builtin_amdgcn_readfirstlane(wave);          // (uniform: chunk indices stay in SGPRs)
        // The sweep (below) walks 64-line chunks; a wave's i-th chunk:
        const int nChunks = (M + kWave - 1) / kWave;
        const int nWaves = NT / kWave;
        // the per-line constants of the NEXT chunk are loaded while this one is computed (loop-carried, so the
        // global-load latency is never exposed between the loops of a chunk)
        struct LineConst { double z, quiet, lowE, x; int bnd; };
        auto chunk_of = [&](int i) { return i * nWaves + ((i & 1) ? (nWaves - 1 - waveU) : waveU); };
        auto load_line = [&](unsigned kc) {               // the constants of line kc < M
            // (byte offsets as 32-bit unsigned values: scalar base + vector offset addressing, no 64-bit address arithmetic)
            const char* lc = reinterpret_cast<const char*>(S.lineC) + kc * (unsigned)sizeof(LineConstants);
            const double2 a = *reinterpret_cast<const double2*>(lc);
            // (lowE and the band, not the entry's padding: a register that is loaded and never read is free for the next
            // value at once, and whoever gets it first has to wait for this load -- in the loop that issued it as a prefetch)
            const double lowE = *reinterpret_cast<const double*>(lc + 16);
            const int bnd = *reinterpret_cast<const int*>(lc + 24);
            const double x = *reinterpret_cast<const double*>(reinterpret_cast<const char*>(X) + kc * 8u);
            return LineConst{a.x, a.y, lowE, x, bnd};
        };
        auto load_consts = [&](int i) { return load_line((unsigned)min(chunk_of(i) * kWave + lane, M - 1)); };
        // ---- band contenders (mono long blocks through the slope nodes; see the sweep): per wave, a lower bound of every
        // band's best ratio among the wave's lines, and the lines that can still reach it.  Both sit in the spectrum area
        // behind the 2^(j/256) table: the spectrum is dead with the barrier above, sc takes < kTabLongOff doubles.
        constexpr bool kContend = LONG && NT == 256 && !EXACT && MODE == 1;
        constexpr int kContCap = kWave;                 // contenders a wave evaluates: one gathered chunk
        constexpr int kContLbOff = kTabLongOff + kExpTabLong, kContIdxOff = kContLbOff + (NT / kWave) * kMaxBands;
        static_assert(!kContend || kContIdxOff + (NT / kWave) * kContCap / 4 <= DIM - 100 + 1, "contender areas: inside the spectrum");
        [[maybe_unused]] unsigned long long* const lbKey =
            reinterpret_cast<unsigned long long*>(smem + 4 * H + kContLbOff) + wave * kMaxBands;
        [[maybe_unused]] unsigned short* const contIdx =
            reinterpret_cast<unsigned short*>(smem + 4 * H + kContIdxOff) + wave * kContCap;
        if constexpr (kContend)
            if (lane < kMaxBands) lbKey[lane] = 0ull;    // (the wave's own: read and written by nobody else, no barrier)
        // ... and those of the wave's FIRST chunk here, two barriers ahead of the sweep: the MDCT lines were written by the
        // kernel before this one and come from HBM, a round trip that the node terms and the scans cover.  (Long blocks: the
        // other shapes are short of registers or of a phase long enough to hide it in.)
        constexpr bool kFirstEarly = LONG && NT == 256;
        [[maybe_unused]] LineConst first{};
        if constexpr (kFirstEarly) first = load_consts(0);
        // ---- which evaluation of the upper-side sum the frame takes (wave-uniform): slope nodes (see kNodeR) when its
        // maskers are many and their slopes lie within reach of R nodes, else the sorted sweep.  Long blocks only.
        constexpr bool kNodes = (DIM == 1024 || DIM == 576) && NT == 256;      // (576: 156 of a transition block's <= 237 maskers)
        constexpr int kNodeMaxMaskers = kNodes ? node_max_maskers(DIM ? DIM : 1024) : 0;
        static_assert(!kNodes || kNodeMaxMaskers >= 128, "slope nodes: too few rows for this block shape");
        [[maybe_unused]] double nodeH = 0.0, nodeS0 = 0.0;               // node spacing / shallowest node (1/TAB bit per Bark)
        bool useNodes = false;
        if constexpr (kNodes) {
            const double lo = order_value(slopeKey[0]), hi = order_value(slopeKey[1]);
            nodeH = fmax((hi - lo) * (1.0 / (kNodeR - 1 - 2 * kNodeMargin)), kNodeHMin * TAB);
            nodeS0 = hi + kNodeMargin * nodeH;
            useNodes = nPeaks >= kNodeMinMaskers && nPeaks <= kNodeMaxMaskers && nodeH <= kNodeHMax * TAB;
        }
        // with nodes their rows take the place of the in-band prefix sums (and of the Bark grid before them), which move
        // behind the masker table
        double* const nodeQ = reinterpret_cast<double*>(pkBin);   // [<= 78][kNodeCols]: from the (dead) peak bins to the log10 table
        double* piH = piHi;
        double* piL = piLo;
        if (kNodes && useNodes) { piH = mt + 4 * nPeaks; piL = piH + (nPeaks + 1); }
        // kWave * kSeg >= the block's maximum number of peaks + 1: 512 >= N/4 in general; a block of DIM lines has at
        // most (DIM - 101) / 2 (13 for the short block: one per lane; 237 for the transition blocks: four; 461 for the long
        // block: eight -- but a frame that takes the slope nodes has at most 308: five.  Besides the shorter serial chain,
        // five entries of 32 bytes per lane put the lanes 160 bytes apart; at 256 bytes all 64 read the same bank)
        constexpr int kSegAny = DIM == 128 ? 1 : DIM == 576 ? 4 : kSmrMaxSeg;
        constexpr int kSegNodes = DIM == 1024 ? 5 : kSegAny;
        static_assert(DIM != 1024 || kWave * kSegNodes > node_max_maskers(1024), "segments of the scans");
        auto scan_sc = [&](auto segC) {
            constexpr int kSeg = decltype(segC)::value;
            double loc[kSeg];
            double run = 0.0;
            const int seg = kWave - 1 - lane;           // lanes take the segments in REVERSE order, so that the suffix
#pragma unroll                                          // over segments is a prefix over lanes (DPP shifts go up)
            for (int i = kSeg - 1; i >= 0; --i) {
                const int m = seg * kSeg + i;
                run += (m < nPeaks) ? mt[4 * m + 3] : 0.0;
                loc[i] = run;
            }
            const double incl = wave_incl_scan(run);    // inclusive prefix over lanes of the segment totals
            const double higher = dpp_shift_or_zero<0x138, 0xf>(incl);      // wave_shr:1 -> exclusive: the higher segments
#pragma unroll
            for (int i = 0; i < kSeg; ++i) {
                const int m = seg * kSeg + i;
                if (m < nPeaks) sc[m] = loc[i] + higher;
            }
            if (lane == 0) sc[nPeaks] = 0.0;
        };
        auto scan_pi = [&](auto segC) {
            // pi[m] = I_0 + ... + I_{m-1} in double-double: the in-band sum of a line is a DIFFERENCE of two
            // prefix sums, and with ~106 bits the difference is exact to far below one ulp of the result even
            // when a loud masker sits in the prefix (dynamic range of I within a frame < 2^50)
            constexpr int kSeg = decltype(segC)::value;
            double hi = 0.0, lo = 0.0, locH[kSeg], locL[kSeg];
#pragma unroll
            for (int i = 0; i < kSeg; ++i) {
                const int m = lane * kSeg + i;
                locH[i] = hi; locL[i] = lo;                            // exclusive within the segment
                dd_add(&hi, &lo, (m < nPeaks) ? mt[4 * m] : 0.0, 0.0);
            }
            double inH = hi, inL = lo;                                  // inclusive prefix scan of the segment totals
#define MRC_DD_SCAN_STEP(CTRL, MASK)                                                           \
            dd_add(&inH, &inL, dpp_shift_or_zero<CTRL, MASK>(inH), dpp_shift_or_zero<CTRL, MASK>(inL));
            MRC_DD_SCAN_STEP(0x111, 0xf) MRC_DD_SCAN_STEP(0x112, 0xf) MRC_DD_SCAN_STEP(0x114, 0xf)
            MRC_DD_SCAN_STEP(0x118, 0xf) MRC_DD_SCAN_STEP(0x142, 0xa) MRC_DD_SCAN_STEP(0x143, 0xc)
#undef MRC_DD_SCAN_STEP
            const double exH = dpp_shift_or_zero<0x138, 0xf>(inH), exL = dpp_shift_or_zero<0x138, 0xf>(inL);   // exclusive
#pragma unroll
            for (int i = 0; i < kSeg; ++i) {
                const int m = lane * kSeg + i;
                if (m <= nPeaks) {
                    double h = exH, l = exL;
                    dd_add(&h, &l, locH[i], locL[i]);
                    piH[m] = h; piL[m] = l;
                }
            }
        };
        auto scan_counts = [&](unsigned short* arr) {
            // per-line masker counts: inclusive prefix sums of the two histograms the table build left
            // (cnt[k] = maskers with fl(z_k - z_m) >= -1/2, nUp[k] = maskers with fl(z_k - z_m) > 1/2)
            const int per2 = (M + kWave) / kWave;                            // entries per lane, covers 0..M
            const int k0 = lane * per2, k1 = min(k0 + per2, M + 1);
            int sum = 0;
            for (int k = k0; k < k1; ++k) sum += arr[k];
            int run = wave_incl_scan(sum) - sum;
            for (int k = k0; k < k1; ++k) {
                run += arr[k];
                arr[k] = (unsigned short)run;
            }
        };
        // ... of a 1024-line block, sixteen counts (eight words) per lane in registers: a prefix inside each word, the running
        // total added to both halves (counts <= 461 < 2^16), the lanes' totals scanned with DPP.  (Entry M -- maskers no line
        // sees -- is not read after the scan and stays as it is.)
        [[maybe_unused]] auto scan_counts_1024 = [&](unsigned short* arr) {
            unsigned* w = reinterpret_cast<unsigned*>(arr) + 8 * lane;
            unsigned x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = w[j];
            unsigned carry = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                unsigned v = x[j] + (x[j] << 16);
                v += carry * 0x10001u;
                x[j] = v;
                carry = v >> 16;
            }
            const unsigned before = (unsigned)(wave_incl_scan((int)carry) - (int)carry) * 0x10001u;
#pragma unroll
            for (int j = 0; j < 8; ++j) w[j] = x[j] + before;
        };
        // The node terms, a masker per thread: lambda_r(theta) in product form (prefix x suffix products of theta - j), the two
        // 2^x, the R terms and the two error-bound terms; the four maskers of a row are lanes 4 j .. 4 j + 3 of a wave and
        // are summed there (two DPP steps); row j + 1 of Q gets the row's total, to be turned into prefix sums by node_scan.
        [[maybe_unused]] auto node_terms = [&]() {
            const double* tab64 = smem + 2 * H - kExpTab;                // 2^(j/64) (the 256-entry table is being staged)
            const double invH = 1.0 / nodeH;
            const double s0q = nodeS0 * ((double)kExpTab / TAB), hq = nodeH * ((double)kExpTab / TAB);   // 1/64 bit per Bark
            if (tid < kNodeCols) nodeQ[tid] = 0.0;                       // row 0: no masker below
            for (int base = waveU * kWave; base < nPeaks; base += NT) {  // (wave-uniform)
                const int m = base + lane;
                const bool valid = m < nPeaks;
                const int mm = min(m, nPeaks - 1);
                const double2 Iz = *reinterpret_cast<const double2*>(mt + 4 * mm);       // (one 16-byte read: see the table's stores)
                const double I = valid ? Iz.x : 0.0, zm = Iz.y, sl = mt[4 * mm + 2];
                const double theta = (nodeS0 - sl) * invH;              // the masker's slope in node units, [margin, R-1-margin]
                double suf[kNodeR];                                      // prod_{j > r} (theta - j)
                suf[kNodeR - 1] = 1.0;
#pragma unroll
                for (int r = kNodeR - 2; r >= 0; --r) suf[r] = suf[r + 1] * (theta - (r + 1));
                const double F0 = I * exp2_tab64<kExpTab>(-s0q, zm, tab64);      // I 2^(-sigma_0 z_m)
                const double gm = exp2_tab64<kExpTab>(hq, zm, tab64);            // 2^(h z_m)
                double G[kNodeCols];
                double F = F0, pre = 1.0, lsum = 0.0;
#pragma unroll
                for (int r = 0; r < kNodeR; ++r) {
                    const double lam = (pre * kNodeW.c[r]) * suf[r];    // lambda_r(theta)
                    G[r] = lam * F;
                    lsum += fabs(lam);
                    F *= gm;
                    pre *= theta - r;
                }
                G[kNodeR] = I * (fabs(pre) * kInvFactorial[kNodeR]);    // I |prod_r (theta - r)| / R!
                G[kNodeR + 1] = lsum * F0;
                const bool store = (lane & 3) == 0 && valid;            // (the row's first masker exists)
                double* rowOut = nodeQ + ((m >> 2) + 1) * kNodeCols;
#pragma unroll
                for (int j = 0; j < kNodeCols; ++j) {
                    double v = G[j];
                    v += dpp_move<0xB1>(v);                              // quad_perm [1,0,3,2]
                    v += dpp_move<0x4E>(v);                              // quad_perm [2,3,0,1]
                    if (store) rowOut[j] = v;
                }
            }
        };
        // Row totals -> prefix sums, in place, by two waves (nine columns each): lane = (seventh of the rows, column); a lane loads
        // its <= 11 rows of the column at once and sums them up in registers; the sevenths of a column get the totals below them
        // by a shift and a three-step scan through ds_bpermute (lane - 9 d holds the same column, d sevenths lower).
        [[maybe_unused]] auto node_scan = [&](int half) {
            static_assert(kNodeCols == 18 && kNodeScanSegs * 9 <= kWave, "columns of the row scan");
            static_assert((node_max_maskers(1024) + kNodeC - 1) / kNodeC <= kNodeScanSegs * kNodeSeg, "rows of the row scan");
            const int nR = (nPeaks + kNodeC - 1) / kNodeC;               // rows 1 .. nR hold totals; row q becomes sum_{m < 4 q}
            const int L = (nR + kNodeScanSegs - 1) / kNodeScanSegs;      // <= kNodeSeg
            const int seg = (lane * 57) >> 9;                            // lane / 9 for lane < 64
            const int col = 9 * half + (lane - 9 * seg);
            const bool live = seg < kNodeScanSegs;
            double v[kNodeSeg];
#pragma unroll
            for (int i = 0; i < kNodeSeg; ++i) {
                const int r = 1 + seg * L + i;
                v[i] = (live && i < L && r <= nR) ? nodeQ[r * kNodeCols + col] : 0.0;
            }
#pragma unroll
            for (int i = 1; i < kNodeSeg; ++i) v[i] += v[i - 1];
            const double tot = v[kNodeSeg - 1];
            // the totals BELOW a seventh: an inclusive scan of the totals shifted up by one seventh.  (Not "inclusive minus
            // own": the rows grow by 2^6 .. 2^9 per Bark, and the small sum of the lower rows would be lost in the subtraction.)
            auto from_below = [&](double x, int d) {
                const int from = 4 * (lane - 9 * d);
                const double y = __hiloint2double(__builtin_amdgcn_ds_bpermute(from, __double2hiint(x)),
                                                  __builtin_amdgcn_ds_bpermute(from, __double2loint(x)));
                return seg >= d ? y : 0.0;
            };
            double off = from_below(tot, 1);
#pragma unroll
            for (int d = 1; d < kNodeScanSegs; d *= 2) off += from_below(off, d);
#pragma unroll
            for (int i = 0; i < kNodeSeg; ++i) {
                const int r = 1 + seg * L + i;
                if (live && i < L && r <= nR) nodeQ[r * kNodeCols + col] = v[i] + off;
            }
        };
        bool scansDone = false;
        if constexpr (kNodes) {
            if (useNodes) {                              // (workgroup-uniform)
                // The node terms by every wave.  With more than NT maskers (more than half of the frames of noise) wave 0 builds
                // the terms of the rest in a second round: the scans that need the masker table only then follow on waves
                // 1 .. 3 without a barrier, and the scan over the rows, which needs every wave's terms, comes behind the barrier
                // on two waves.  Otherwise all scans run side by side behind the barrier.  (What a barrier-delimited phase
                // costs is its LONGEST wave: the others hold their slots idle.)
                MRC_PHASE(13);
                node_terms();
                MRC_PHASE(14);
                using SegN = std::integral_constant<int, kSegNodes>;
                auto counts = [&](unsigned short* arr) {
                    if constexpr (DIM == 1024) scan_counts_1024(arr); else scan_counts(arr);
                };
                if (nPeaks > NT) {   // (workgroup-uniform) wave 0 has had a second round of terms
                    if (waveU == 1) scan_pi(SegN{});
                    else if (waveU == 2) { scan_sc(SegN{}); counts(cntArr); }
                    else if (waveU == 3) counts(nUpArr);
                    MRC_PHASE(9);                        // (profiling build: the slot of the sorted sweep's near field)
                    __syncthreads();
                    MRC_PHASE(15);
                    if (waveU == 2 || waveU == 3) node_scan(waveU - 2);
                } else {                                 // every wave is through with its terms at the same time
                    __syncthreads();
                    MRC_PHASE(15);
                    if (waveU < 2) node_scan(waveU);
                    else if (waveU == 2) scan_pi(SegN{});
                    else { scan_sc(SegN{}); counts(cntArr); counts(nUpArr); }
                    MRC_PHASE(9);
                }
                scansDone = true;
            }
        }
        if (!scansDone) {
            // four independent scans, dealt to the workgroup's waves (4 waves: one each; 2 waves: two each)
            for (int task = waveU; task < 4; task += NT / kWave) {
                using SegA = std::integral_constant<int, kSegAny>;
                if (task == 0) scan_sc(SegA{});
                else if (task == 1) scan_pi(SegA{});
                else if constexpr (DIM == 1024) scan_counts_1024(task == 2 ? cntArr : nUpArr);
                else scan_counts(task == 2 ? cntArr : nUpArr);
            }
        }
        __syncthreads();
        MRC_PHASE(5); MRC_STOP(5);

        // Each wave sweeps 64-line chunks (one line per lane); the chunk order pairs cheap (low) with
        // expensive (high) chunks so the four waves finish together.  Per line, the Bark-sorted maskers
        // split into [0, nUp): more than 1/2 Bark below the line (upper slope, needs 2^x),
        // [nUp, cnt): within +-1/2 Bark (contributes exactly I_m), [cnt, P): more than 1/2 Bark above
        // (lower slope, served by the suffix sums).
        // in-band maskers [from, cnt) and the lower side on top of `tot` (quiet threshold + upper side): the line's masked intensity
        auto tail_sum = [&](double tot, int cnt, int from, double lowE) {
            if (cnt > from) {
                // sum of I_m over [from, cnt) = pi[cnt] - pi[from], in double-double
                const double ah = piH[cnt], al = piL[cnt], bh = piH[from], bl = piL[from];
                const double d1 = ah - bh;
                const double v = d1 - ah;
                const double e = ((ah - (d1 - v)) - (bh + v)) + (al - bl);
                tot += d1 + e;
            }
            // maskers more than 1/2 Bark above the line: -27 dB/Bark for all of them
            return fma(lowE, sc[cnt], tot);
        };
        // psychoac.py:173,212-217: SMR of a band = max over its lines of SPL(4 xs^2) - 6 scale - SPL(t).  Unless one
        // of the two SPLs sits on its -30 dB floor (digital silence) that is 10 log10(4 xs^2 / t) - 6 scale, and
        // log10 is monotone: the band maximum of the RATIO is taken and converted once per band at the end
        // instead of two log10 per line (the difference to the reference's order of roundings is ~1e-14 dB, five
        // orders below what the FFT in front of it already differs by).  Lines on the floor, and every line when
        // the caller wants the thresholds themselves, take the reference's formula.  (Lines under an infinite threshold:
        // line_ratio.)
        // (a2 of a line: the intensity of its own MDCT line, psychoac.py:212)
        // = 2 xs^2 / (1/2) with xs = x 2^scale (codecThem.py:323; psychoac.py:212): the factors of two commute with the one
        // rounding of the square, so the square of 2 xs is the same double
        auto line_a2 = [&](const LineConst& cur) {
            const double xs2 = ldexp(cur.x, scale + 1);
            return xs2 * xs2;
        };
        auto line_plain = [&](double a2, double t) { return thresh != nullptr || !(a2 >= kSplFloorGuard && t >= kSplFloorGuard); };
        // noPlain: the caller has checked that no lane of the chunk takes the reference's formula (no call in its loop)
        auto finish = [&](const LineConst& cur, int k, double t, auto noPlain) {
            const double a2 = line_a2(cur);
            const bool plain = decltype(noPlain)::value ? false : line_plain(a2, t);
            double ex = -1e300, q = 0.0;
            if (plain) {
                double thr;
                ex = excess_plain(t, a2, scale, logTab, &thr);
                if (thresh && k < M) thresh[(int64_t)unit * M + k] = thr;
            } else {
                q = line_ratio(a2, t);
            }
            const int bnd = cur.bnd;                     // lanes past the end repeat the last line: maxima unchanged
            if (__all(bnd == __builtin_amdgcn_readfirstlane(bnd))) {
                // whole chunk inside one band (the wide top bands): 64 lanes on one LDS address would be served one by
                // one; the maximum of each 16-lane row is taken in registers and four lanes go to the LDS
                const bool rowHead = (lane & 15) == 0;
                const double qBest = row_max(q);
                if (rowHead) atomicMax(&ratioKey[bnd], (unsigned long long)__double_as_longlong(qBest));
                if (__any(plain)) {
                    const double best = row_max(ex);
                    if (rowHead) atomicMax(&bandKey[bnd], order_key(best));
                }
                if (wantPeak) {
                    const double pk = row_max(fabs(cur.x));
                    if (rowHead) atomicMax(&peakKey[bnd], (unsigned long long)__double_as_longlong(pk));
                }
            } else {
                atomicMax(&ratioKey[bnd], (unsigned long long)__double_as_longlong(q));
                if (plain) atomicMax(&bandKey[bnd], order_key(ex));
                if (wantPeak) atomicMax(&peakKey[bnd], (unsigned long long)__double_as_longlong(fabs(cur.x)));
            }
        };
        __builtin_amdgcn_s_setprio(0);
        const double slMid = 0.5 * (order_value(slopeKey[0]) + order_value(slopeKey[1]));
        const double spreadHalf = 0.5 * (order_value(slopeKey[1]) - order_value(slopeKey[0])) * (0.6931471805599453094 / TAB);
        if (kNodes && useNodes) {
            if constexpr (kNodes) {
            // ---- slope nodes: per line two 2^x, a Horner pass over its row of prefix sums, and the direct pairs of the
            // maskers between the row and nUp
            MRC_NODE_COUNT(0);
            const double xr = (nodeH * kNodeR) / (-nodeS0);
            double ps = xr * xr;
            ps *= ps; ps *= ps; ps *= ps;                // (h R / |sigma_0|)^16
            const double psiStar = ps * kExpMinus16;
            // The chunks where the evaluation below is not the last word -- a line whose error bound fails, a line on the
            // SPL floor, every chunk when the caller wants the thresholds -- are set aside (a bit per chunk of the wave) and
            // done after the loop: the out-of-line calls they need would otherwise sit in the hot loop and cost it the
            // scalar registers a call clobbers (its pointers and masks were being reloaded from a spill lane every chunk).
            struct NodeEval { double t, bound; int cnt, nUp; };
            auto node_chunk = [&](const LineConst& cur, int kc) {
                const int cnt = cntArr[kc], nUp = nUpArr[kc];      // maskers that reach the line / lie > 1/2 Bark below it
                const double zq = cur.z - 0.5;
                const int q = nUp >> 2, rem = nUp & 3;   // (kNodeC = 4)
                const double* row = nodeQ + q * kNodeCols;
                const double E0 = exp2_tab64<TAB>(nodeS0, zq, e2tab);
                const double g = exp2_tab64<TAB>(-nodeH, zq, e2tab);
                const double errBound = fma(psiStar, row[kNodeR], (kNodeRoundEps * E0) * row[kNodeR + 1]);
                const double up = node_line<kNodeC - 1, TAB>(row, mt, e2tab, 4 * q, rem, nPeaks - 1, zq, E0, g);
                return NodeEval{tail_sum(cur.quiet + up, cnt, nUp, cur.lowE), errBound, cnt, nUp};
            };
            unsigned setAside = 0;                       // (wave-uniform)
            LineConst nxt = kFirstEarly ? first : load_consts(0);
            if constexpr (kContend) {
                // ---- band contenders.  A band's SMR is the maximum of a2 / t over its lines, and t = quiet + in-band + lower
                // side + upper side with every term positive.  What tail_sum adds to the quiet threshold alone is a lower
                // bound t_lb of t; with E0 times the row's column R + 1 (sum of Lambda_m I_m 2^(-sigma_0 z_m), Lambda_m >= 1,
                // sigma_0 >= every slope, over at least the maskers below the line) on top it is an upper bound t_ub.  The wave
                // takes, per band, L = max of a2 / t_ub over ITS lines -- a ratio one of them reaches in the evaluation -- and
                // evaluates only the lines with a2 >= L t_lb, gathered into one chunk.  The margins (kShrinkLb on L, kShrink
                // on the comparison) cover the roundings of either bound, of the reciprocal and the node tolerance: a line
                // left out is strictly below a line that is evaluated, by the same arithmetic as before, so the integer
                // maxima end as they did.
                // Chunks with a line near the SPL floor go through the set-aside path whole, as before; so does the original
                // chunk of a contender whose error bound fails, and all four when the contenders do not fit.
                // The bounds themselves only have to be SAFE, so the pass that forms them for all 1024 lines does without the
                // accuracy the evaluation needs.  With mu = 2^-50 piH[cnt] (>= 4 ulp of either prefix sum) and d = fl(piH[cnt] -
                // piH[nUp]) of the high parts alone, and t the sum that the evaluation's value stands for (it lies within the node
                // tolerance, 1e-13, of it; 2^-30 and 2^-13 below have room for that):
                //   in-band sum S as tail_sum forms it:  d - mu <= S <= d + mu   (the two low parts are each below half an ulp
                //       of their high part, d's own rounding is another half; S >= 0)
                //   t_lb = quiet + max(d - mu, 0) + lowE sc[cnt]   <= t (1 + 2^-50)      (three roundings)
                //   E0'  = exp2_tab_above (the table entry above the exponent)  >= E0 (1 - 2^-52), at most 0.41 % above it
                //   t_ub = t_lb + 2 mu + E0' col[R + 1]            >= t (1 - 2^-50)
                //   r    = v_rcp_f64(t_ub) without a Newton step: within kRcpRel of 1 / t_ub.  recip_nr reaches its 2^-52
                //       after two steps, each of which squares the error, from an estimate within 2^-13; twice that is taken.
                //   lb   = a2 r kShrinkLb  <  a2 / t_ub (1 - 2^-13)  <  a2 recip_nr(t)   (kShrinkLb = 1 - 2 kRcpRel)
                // so the band's L = max lb stays strictly below the ratio its line reaches in the evaluation, and a line with
                // a2 < L t_lb kShrink has a2 recip_nr(t) < L (1 - 2^-31): strictly below that line, as before.  A looser bound
                // only lets more lines through to the evaluation, which is tail_sum, node_chunk and line_ratio untouched.
                constexpr double kShrink = 1.0 - 0x1p-30, kFloorHi = kSplFloorGuard * (1.0 + 0x1p-30);
                constexpr double kRcpRel = 0x1p-12, kShrinkLb = 1.0 - 2 * kRcpRel, kInBandMargin = 0x1p-50;
                static_assert(NT / kWave == 4 && DIM / kWave == 16, "a wave's chunks: four, the i-th in lines [256 i, 256 i + 256)");
                double a2s[4], tlb[4];
                int bnds[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int k = chunk_of(i) * kWave + lane;
                    const LineConst cur = nxt;
                    if (i < 3) nxt = load_consts(i + 1);
                    MRC_PHASE(i == 0 ? 25 : 6);
                    const int cnt = cntArr[k], nUp = nUpArr[k];
                    const double a2 = line_a2(cur);
                    const double ah = piH[cnt];
                    const double d = ah - piH[nUp], mu = ah * kInBandMargin;
                    const double tl = fma(cur.lowE, sc[cnt], cur.quiet + fmax(d - mu, 0.0));
                    const int bnd = cur.bnd;
                    const bool oneBand = __all(bnd == __builtin_amdgcn_readfirstlane(bnd));
                    const bool rowHead = (lane & 15) == 0;
                    const bool whole = __any(!(a2 >= kFloorHi && tl >= kFloorHi));
                    a2s[i] = a2; tlb[i] = tl; bnds[i] = bnd;
                    double lb = 0.0;
                    if (whole) setAside |= 1u << i;
                    else {
                        const double E0 = exp2_tab_above<TAB>(nodeS0, cur.z - 0.5, e2tab);
                        const double tub = fma(E0, nodeQ[((nUp + kNodeC - 1) >> 2) * kNodeCols + kNodeR + 1], tl + (mu + mu));
                        lb = (a2 * __builtin_amdgcn_rcp(tub)) * kShrinkLb;
                    }
                    // (every line's |X| goes into the band peaks here; the band's bound from the lines of this chunk)
                    if (oneBand) {
                        const double pk = row_max(fabs(cur.x));
                        if (rowHead) atomicMax(&peakKey[bnd], (unsigned long long)__double_as_longlong(pk));
                        if (!whole) {
                            const double best = row_max(lb);
                            if (rowHead) atomicMax(&lbKey[bnd], (unsigned long long)__double_as_longlong(best));
                        }
                    } else {
                        atomicMax(&peakKey[bnd], (unsigned long long)__double_as_longlong(fabs(cur.x)));
                        if (!whole) atomicMax(&lbKey[bnd], (unsigned long long)__double_as_longlong(lb));
                    }
                    MRC_PHASE(8);
                }
                // (the wave's lanes read what other lanes of it wrote, here and below: ordered within the wavefront)
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                int nCont = 0;                           // (wave-uniform)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if ((setAside >> i) & 1u) continue;
                    const double L = __longlong_as_double((long long)lbKey[bnds[i]]);
                    const bool in = !(a2s[i] < (L * tlb[i]) * kShrink);
                    const unsigned long long m = __ballot(in);
                    const int pos = nCont + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                    if (in && pos < kContCap) contIdx[pos] = (unsigned short)(chunk_of(i) * kWave + lane);
                    nCont += __popcll(m);
                }
                if (nCont > kContCap) { setAside = 0xFu; nCont = 0; }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                if (nCont > 0) {
                    const int k = contIdx[min(lane, nCont - 1)];       // (lanes past the end repeat the last one: maxima unchanged)
                    const LineConst cur = load_line((unsigned)k);
                    const NodeEval ev = node_chunk(cur, k);
                    const bool bad = !(ev.bound <= kNodeTol * ev.t);
                    if (__any(bad)) {                     // (rare) the contender's own chunk goes to the sorted sweep: none of
#pragma unroll                                            // its lines counts here
                        for (int i = 0; i < 4; ++i)
                            if (__any(bad && (k >> 8) == i)) setAside |= 1u << i;
                    }
                    MRC_NODE_COUNT(2);
                    const bool live = !((setAside >> (k >> 8)) & 1u);
                    const double q = live ? line_ratio(line_a2(cur), ev.t) : 0.0;
                    atomicMax(&ratioKey[cur.bnd], (unsigned long long)__double_as_longlong(q));
                    MRC_PHASE(10);
                }
            } else
            for (int i = 0; chunk_of(i) < nChunks; ++i) {
                const int k = chunk_of(i) * kWave + lane;
                const LineConst cur = nxt;
                nxt = load_consts(i + 1);
                if (haveSwitch && !__any(needBand[cur.bnd])) continue;                           // (see needBand)
                MRC_PHASE(i == 0 ? 25 : 6);                     // (25: the wave's first chunk -- its loads are `first`, not the loop's prefetch)
                const NodeEval ev = node_chunk(cur, min(k, M - 1));
                MRC_PHASE(8);
                const bool odd = !(ev.bound <= kNodeTol * ev.t) || line_plain(line_a2(cur), ev.t);
                if (__any(odd)) { setAside |= 1u << i; continue; }
                MRC_NODE_COUNT(2);
                finish(cur, k, ev.t, std::true_type{});
                MRC_PHASE(10);
            }
            while (setAside) {
                const int i = __builtin_ctz(setAside);
                setAside &= setAside - 1;
                const int c = chunk_of(i);
                const int k = c * kWave + lane;
                const LineConst cur = load_consts(i);
                const NodeEval ev = node_chunk(cur, min(k, M - 1));
                double t = ev.t;
                if (__any(!(ev.bound <= kNodeTol * ev.t))) {
                    // a line of this chunk lives on what the interpolation does worst: the chunk goes back to the sorted sweep
                    MRC_NODE_COUNT(3);
                    if (sens && lane == 0) atomicAdd(&sens[4], 1ull);
                    const double tot = cur.quiet + upper_cold<TAB>(mt, e2tab, S.zb, M, c, lane, ev.nUp, ev.cnt, cur.z, slMid, spreadHalf);
                    t = tail_sum(tot, ev.cnt, __builtin_amdgcn_readlane(ev.nUp, kWave - 1), cur.lowE);
                } else {
                    MRC_NODE_COUNT(2);
                }
                finish(cur, k, t, std::false_type{});
            }
            }
        } else {
        // ---- sorted sweep.  Rounds of up to four chunks per wave.  Pass 1 evaluates the FAR FIELD of the round's chunks --
        // the only part that needs a large register tile (the expansion coefficients) -- and keeps one value per line; pass 2
        // does the near maskers, the in-band and lower-side sums and the SPL conversions with that value added in.
        MRC_NODE_COUNT(1);
        for (int i0 = 0; chunk_of(i0) < nChunks; i0 += 4) {
        __builtin_amdgcn_s_setprio(kFarPrio);
        double far0 = 0.0, far1 = 0.0, far2 = 0.0, far3 = 0.0;
        unsigned farMask = 0;                            // bit u: chunk u of the round took the far field
        // (a block of DIM lines has at most (DIM - 101) / 2 maskers: a short block's 13 never reach kFarMinMaskers, so its
        // instance carries no far-field code -- and fits the registers of eight waves per SIMD)
        constexpr bool kHaveFar = DIM == 0 || (DIM - 101) / 2 >= kFarMinMaskers;
        for (int u = 0; kHaveFar && u < 4; ++u) {
            const int c = chunk_of(i0 + u);
            if (c >= nChunks) break;
            const int kc = min(c * kWave + lane, M - 1);
            if (haveSwitch && !__any(needBand[S.bandOfLine[kc]])) continue;                      // (see needBand)
            const int nFar = __builtin_amdgcn_readfirstlane((int)nUpArr[kc]);      // nUp of the chunk's first line
            double acc = 0.0;
            if (!far_eval<TAB, kHaveFar>(mt, e2tab, S.zb, M, c, lane, nFar, S.zb[kc], slMid, spreadHalf, &acc)) continue;
            farMask |= 1u << u;
            far0 = u == 0 ? acc : far0;
            far1 = u == 1 ? acc : far1;
            far2 = u == 2 ? acc : far2;
            far3 = u == 3 ? acc : far3;
        }
        MRC_PHASE(7);
        // ---- pass 2
        __builtin_amdgcn_s_setprio(0);
        LineConst nxt = (kFirstEarly && i0 == 0) ? first : load_consts(i0);
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u;
            const int c = chunk_of(i);
            if (c >= nChunks) break;
            const int k = c * kWave + lane;
            const int kc = min(k, M - 1);
            const LineConst cur = nxt;
            nxt = load_consts(i + 1);
            if (haveSwitch && !__any(needBand[cur.bnd])) continue;                               // (see needBand)
            // quiet threshold + far field (psychoac.py:155,166-168; the order of the additions is free, see above)
            double tot = cur.quiet + (u == 0 ? far0 : u == 1 ? far1 : u == 2 ? far2 : far3);
            const int cnt = cntArr[kc], nUp = nUpArr[kc];      // maskers that reach the line / lie > 1/2 Bark below it
            MRC_PHASE(6);
            tot = near_eval<TAB>(mt, e2tab, nUp, cnt, cur.z - 0.5, ((farMask >> u) & 1u) != 0, tot);
            MRC_PHASE(9);
            if (MRC_PROFILE_SKIP & 8) {
                if (tot + cur.lowE + cur.x == 12345.0 && cur.bnd == 77) bandKey[0] = 1;      // keep the loads alive
                continue;
            }
            // no line of the chunk is above the band of the maskers from max nUp on: a line that sees one is inside +-1/2 Bark
            finish(cur, k, tail_sum(tot, cnt, __builtin_amdgcn_readlane(nUp, kWave - 1), cur.lowE), std::false_type{});
            MRC_PHASE(10);
        }
        }
        }
    }
    __syncthreads();
    MRC_PHASE(11);
#ifdef MRC_PROFILE_PHASES
    __syncthreads();
    if (tid < 32 && (blockIdx.x & 63) == 0) atomicAdd(&gPhaseCycles[tid], tid == 31 ? 1ull : sPhase_[tid]);   // [31]: workgroups sampled
#endif
    for (int bnd = tid; bnd < S.nBands; bnd += NT) {
        double v = bandKey[bnd] ? order_value(bandKey[bnd]) : -1e300;              // lines on the SPL floor / EXACT
        if (!EXACT && ratioKey[bnd]) {
            const double q = __longlong_as_double((long long)ratioKey[bnd]);
            v = fmax(v, 10 * log10_tab32(q, logTab) - 6. * scale);
        }
        smr[(int64_t)unit * S.nBands + bnd] = v;
        // max |X| per band of the UNSCALED lines: what the scale factors need (codecThem.py:346), so the back end
        // does not have to read the lines once more for it
        if (wantPeak) bandPeak[(int64_t)unit * S.nBands + bnd] = __longlong_as_double((long long)peakKey[bnd]);
    }
}

template <bool EXACT, class SampleT, int NT, int DIM, int MODE>
__global__ __launch_bounds__(NT)
__attribute__((amdgpu_waves_per_eu(DIM == 128 ? kSmrWavesPerSimdShort : kSmrWavesPerSimd,
                                   DIM == 128 ? kSmrWavesPerSimdShort : kSmrWavesPerSimd))) void smr_kernel(DevShape S, int nsigArg, const SampleT* __restrict__ chL,
                                                       const SampleT* __restrict__ chR, int64_t stride,
                                                       const int64_t* __restrict__ offsetsArg,
                                                       const double* __restrict__ lines,
                                                       const int* __restrict__ oscale, double* __restrict__ smr,
                                                       double* __restrict__ threshArg, double* __restrict__ bandPeakArg,
                                                       const int* __restrict__ msSwitch, SmrLds layArg,
                                                       unsigned long long* __restrict__ sens) {
    smr_body<EXACT, SampleT, NT, DIM, MODE>(S, nsigArg, chL, chR, stride, offsetsArg, lines, oscale, smr, threshArg,
                                            bandPeakArg, msSwitch, layArg, sens);
}

// dynamic LDS (doubles): FFT ping-pong [4H] + intensity spectrum [peakLast + 1].  The staged tables go into
// areas that are dead when they are needed if there is room (the long block is sized for 4 workgroups per CU
// and must not grow), else behind the spectrum.
inline SmrLds smr_launch_layout(const DevShape& S, size_t* ldsBytes) {
    int total = 0;
    const SmrLds lay = smr_layout(S.H, S.halfN, S.peakLast, &total);
    *ldsBytes = (size_t)total * sizeof(double);
    return lay;
}

}  // namespace
}  // namespace mrc
