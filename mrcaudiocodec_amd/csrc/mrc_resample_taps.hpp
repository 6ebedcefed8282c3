// The filter of mrc_pac_store_decode_window_resampled, on the host alone: the argument rule, the taps (mrc_resample_taps) and
// the choice of resample_out_kernel's LDS layout.  Nothing here touches a handle, the HIP runtime or a device, so the file
// compiles into a stand-alone host program (tests/resample_taps_check.cpp) that a sanitizer can see whole.
//
// up / down, reduced by their gcd, is the output rate over the input rate.  base = min(1, up / down) * rolloff is the
// cut-off as a fraction of the input's Nyquist frequency, W = ceil(zeros / base) (both in double) the filter's half width in
// input samples.  Phase p, tap j, with d = (j - W + 1) - p / up and t = base * d:
//   taps[p][j] = base * sinc(t) * cos^2(pi t / (2 zeros))  for |t| < zeros, else 0;   sinc(t) = sin(pi t) / (pi t), 1 at 0
// -- a Hann-windowed sinc -- evaluated in long double and rounded to double once.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <string>

namespace mrc {

constexpr int kResampleMaxTerm = 1024, kResampleMaxRatio = 8, kResampleMaxZeros = 64;

struct ResampleSpec {
    int up = 0, down = 0, zeros = 0;     // up / down reduced
    double rolloff = 0.0;
    int W = 0;                           // half width: a row holds 2 W taps (at most 2048)
};

// the refusal's words (the caller puts its own name in front), empty if there is none; *out is then filled
inline std::string resample_spec(int up, int down, int zeros, double rolloff, ResampleSpec* out) {
    if (up < 1) return "up " + std::to_string(up) + " is not positive";
    if (down < 1) return "down " + std::to_string(down) + " is not positive";
    const int g = std::gcd(up, down);
    up /= g;
    down /= g;
    const std::string ratio = std::to_string(up) + " / " + std::to_string(down);
    if (up > kResampleMaxTerm) return "up " + std::to_string(up) + " (of " + ratio + ", reduced) is above " + std::to_string(kResampleMaxTerm);
    if (down > kResampleMaxTerm) return "down " + std::to_string(down) + " (of " + ratio + ", reduced) is above " + std::to_string(kResampleMaxTerm);
    if (up == down) return "up / down is 1: there is nothing to resample (up " + std::to_string(up * g) + ", down " + std::to_string(down * g) + ")";
    if (down > kResampleMaxRatio * up) return "down " + std::to_string(down) + " is above 8 * up (" + ratio + ", reduced)";
    if (up > kResampleMaxRatio * down) return "up " + std::to_string(up) + " is above 8 * down (" + ratio + ", reduced)";
    if (zeros < 1 || zeros > kResampleMaxZeros) return "zeros " + std::to_string(zeros) + " is outside 1.." + std::to_string(kResampleMaxZeros);
    if (!(rolloff >= 0.5 && rolloff <= 1.0)) return "rolloff " + std::to_string(rolloff) + " is outside [0.5, 1]";
    const double base = std::min(1.0, (double)up / (double)down) * rolloff;
    *out = ResampleSpec{up, down, zeros, rolloff, (int)std::ceil((double)zeros / base)};
    return std::string();
}

// taps [up][2 W] of a spec resample_spec filled
inline void resample_taps(const ResampleSpec& r, double* taps) {
    const long double pi = 3.14159265358979323846264338327950288L;
    const long double base = (long double)std::min(1.0, (double)r.up / (double)r.down) * (long double)r.rolloff;
    for (int p = 0; p < r.up; ++p)
        for (int j = 0; j < 2 * r.W; ++j) {
            const long double d = (long double)(j - r.W + 1) - (long double)p / (long double)r.up, t = base * d;
            long double v = 0.0L;
            if (std::fabs(t) < (long double)r.zeros) {
                const long double c = std::cos(pi * t / (2.0L * (long double)r.zeros));
                v = base * (t == 0.0L ? 1.0L : std::sin(pi * t) / (pi * t)) * c * c;
            }
            taps[(size_t)p * (size_t)(2 * r.W) + (size_t)j] = (double)v;
        }
}

// resample_out_kernel's fold reads, at every tap, one double of the staged run per lane with a 64-bit LDS read: such a read is
// served in two halves of 32 lanes over 32 banks of one double, equal addresses broadcast, and n different doubles on one bank
// cost n cycles.  Lane k of a half reads run index o + floor((p0 + k g down) / up): g = 1 when a half takes 32 consecutive
// outputs, 2 when the wave's two halves take the even and the odd outputs; double i is kept at i + skew * (i >> 5) (skew 1:
// one double of padding per bank row).  -> the cycles such a read takes -- the largest number of different doubles on one
// bank -- as the mean over every phase p0 of the half's first output and every alignment o of the run: 1.0 is conflict-free.
inline double resample_lds_cycles(int up, int down, int g, int skew) {
    int64_t sum = 0;
    for (int p0 = 0; p0 < up; ++p0)
        for (int o = 0; o < 32; ++o) {
            int onBank[32] = {}, before = -1, worst = 1;     // (the indices do not decrease with k: equal ones are neighbours)
            for (int k = 0; k < 32; ++k) {
                const int i = o + (int)(((int64_t)p0 + (int64_t)k * g * down) / up);
                if (i != before) worst = std::max(worst, ++onBank[(i + skew * (i >> 5)) & 31]);
                before = i;
            }
            sum += worst;
        }
    return (double)sum / (32.0 * up);
}

// the layout with the fewest cycles, the plainest first among equals
inline void resample_lds_layout(int up, int down, int* g, int* skew) {
    double best = 1e30;
    for (int cand = 0; cand < 4 && best > 1.0; ++cand) {
        const int cg = 1 + (cand >> 1), cs = cand & 1;
        const double deg = resample_lds_cycles(up, down, cg, cs);
        if (deg < best) {
            best = deg;
            *g = cg;
            *skew = cs;
        }
    }
}

}  // namespace mrc
