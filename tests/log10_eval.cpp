// CPU side of tests/test_gpu_helper_probes.py::test_spl_db_tab_and_log10: mrc_log10.hpp (the same source the device code
// compiles) on the doubles read from stdin, raw 8-byte values in and out, for a bit-for-bit comparison with the device.
#include "mrc_log10.hpp"
#include <cstdio>

int main() {
    double tab[mrc::kLogTabEntries * 4] = {};
    for (int j = 0; j < mrc::kLogTabEntries; ++j)
        for (int c = 0; c < 3; ++c) tab[4 * j + c] = mrc::kLog10Tab[j][c];
    double x;
    while (std::fread(&x, sizeof x, 1, stdin) == 1) {
        const double y = mrc::log10_tab32(x, tab);
        std::fwrite(&y, sizeof y, 1, stdout);
    }
    return 0;
}
