// Host-only check of mrcaudiocodec_amd/csrc/mrc_resample_taps.hpp (tests/test_store_resample_cpu.py compiles it, with
// AddressSanitizer and UndefinedBehaviorSanitizer where g++ has them): the argument rule, the taps' shape written into a
// buffer of exactly up * 2 W doubles, and the LDS layout choice against cases worked out by hand.  Says nothing and exits 0
// when all is well; with the argument "layouts" it prints the layout and its conflict degree for a list of ratios.
#include "mrc_resample_taps.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace mrc;

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);          \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

int main(int argc, char** argv) {
    const int ratios[][2] = {{1, 3}, {2, 3}, {3, 2}, {160, 441}, {320, 441}, {147, 160}, {160, 147}, {1, 8}, {8, 1},
                             {1, 2}, {1, 4}, {3, 4}, {5, 8}, {1024, 1023}, {1023, 1024}, {128, 1023}};
    if (argc > 1 && !std::strcmp(argv[1], "layouts")) {
        for (const auto& r : ratios) {
            int g = 1, skew = 0;
            resample_lds_layout(r[0], r[1], &g, &skew);
            std::printf("%4d / %-4d plain %.2f cycles; chosen: %s%s, %.2f\n", r[0], r[1], resample_lds_cycles(r[0], r[1], 1, 0),
                        g == 2 ? "evenOdd" : "consecutive", skew ? " + skew" : "", resample_lds_cycles(r[0], r[1], g, skew));
        }
        return 0;
    }
    ResampleSpec s;
    // ---- the rule
    CHECK(resample_spec(4, 6, 16, 0.9475, &s).empty() && s.up == 2 && s.down == 3 && s.W == 26);
    CHECK(resample_spec(1, 8, 64, 0.5, &s).empty() && s.W == 1024);
    CHECK(resample_spec(2048, 2049 * 2, 16, 0.9, &s).find("down") != std::string::npos);
    CHECK(resample_spec(0, 3, 16, 0.9, &s).find("up 0") != std::string::npos);
    CHECK(resample_spec(3, -1, 16, 0.9, &s).find("down -1") != std::string::npos);
    CHECK(resample_spec(5, 5, 16, 0.9, &s).find("up / down is 1") != std::string::npos);
    CHECK(resample_spec(1, 9, 16, 0.9, &s).find("down 9") != std::string::npos);
    CHECK(resample_spec(9, 1, 16, 0.9, &s).find("up 9") != std::string::npos);
    CHECK(resample_spec(1, 3, 0, 0.9, &s).find("zeros 0") != std::string::npos);
    CHECK(resample_spec(1, 3, 65, 0.9, &s).find("zeros 65") != std::string::npos);
    CHECK(resample_spec(1, 3, 16, 0.49, &s).find("rolloff") != std::string::npos);
    CHECK(resample_spec(1, 3, 16, std::nan(""), &s).find("rolloff") != std::string::npos);
    // ---- the taps fill exactly up * 2 W doubles (a heap buffer of that size: the sanitizer sees an overrun)
    for (const auto& r : ratios)
        for (int zeros : {1, 6, 16, 64}) {
            CHECK(resample_spec(r[0], r[1], zeros, 0.9475, &s).empty());
            std::vector<double> t((size_t)s.up * 2 * s.W, 7.0);
            resample_taps(s, t.data());
            double sum = 0.0;
            for (int j = 0; j < 2 * s.W; ++j) sum += t[j];
            CHECK((zeros < 6 || std::fabs(sum - 1.0) < 1e-3) && t[(size_t)s.W - 1] > 0.0 && t.back() != 7.0);
            for (int j = 0; j + 1 < 2 * s.W; ++j) CHECK(t[j] == t[2 * s.W - 2 - j]);           // row 0 about j = W - 1
            for (int p = 1; p < s.up; ++p)
                for (int j = 0; j < 2 * s.W; j += 3)
                    CHECK(std::fabs(t[(size_t)p * 2 * s.W + j] - t[(size_t)(s.up - p) * 2 * s.W + (2 * s.W - 1 - j)]) < 1e-15);
        }
    // ---- the LDS layout: by hand
    CHECK(resample_lds_cycles(1, 1, 1, 0) == 1 && resample_lds_cycles(3, 2, 1, 0) == 1);     // down <= up: 32 banks
    CHECK(resample_lds_cycles(1, 3, 1, 0) == 1 && resample_lds_cycles(1, 5, 1, 0) == 1);     // odd strides
    CHECK(resample_lds_cycles(1, 2, 1, 0) == 2 && resample_lds_cycles(1, 4, 1, 0) == 4 && resample_lds_cycles(1, 8, 1, 0) == 8);
    CHECK(resample_lds_cycles(1, 2, 1, 1) < 2 && resample_lds_cycles(1, 4, 1, 1) < 2 && resample_lds_cycles(1, 8, 1, 1) < 2);
    CHECK(resample_lds_cycles(2, 3, 1, 0) == 2 && resample_lds_cycles(2, 3, 2, 0) == 1);     // 3 / 2: the halves' stride 3
    for (const auto& r : ratios) {
        int g = 0, skew = -1;
        resample_lds_layout(r[0], r[1], &g, &skew);
        CHECK((g == 1 || g == 2) && (skew == 0 || skew == 1));
        CHECK(resample_lds_cycles(r[0], r[1], g, skew) <= resample_lds_cycles(r[0], r[1], 1, 0));
    }
    return failures ? 1 : 0;
}
