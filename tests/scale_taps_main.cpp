// The table builder of libfldr_scale.so (fldr-vfi_amd/scale/scale_taps.h) as a stand-alone host program, for the host sanitizers:
//   g++ -std=c++17 -fsanitize=undefined,address -Iinclude -Ifldr-vfi_amd/scale tests/scale_taps_main.cpp && ./a.out
// It builds the tables of sizes 1 and 16384, of the ratios at both tap limits and of every filter and kind into buffers of exactly the
// documented size (so that a write past them is seen), and checks each row's sum.  tests/test_scale_cpu.py builds and runs it.
#include <cstdio>
#include <vector>

#include "scale_taps.h"

static int check(int in, int out, int filter, int kind) {
    const int n = scale_taps_count(in, out, filter);
    if (n < 0) return n;
    const int outputs = scale_outputs(out, kind);
    std::vector<int32_t> left((size_t)outputs);
    std::vector<int16_t> coef((size_t)outputs * n);
    const int rc = scale_taps(in, out, filter, kind, left.data(), coef.data());
    if (rc) return rc;
    for (int o = 0; o < outputs; ++o) {
        int sum = 0, mag = 0;
        for (int k = 0; k < n; ++k) { sum += coef[(size_t)o * n + k]; mag += abs(coef[(size_t)o * n + k]); }
        if (sum != 16384 || mag > 32767) { printf("row %d of %d -> %d filter %d kind %d: sum %d, sum|q| %d\n", o, in, out, filter, kind, sum, mag); return 1; }
        if (o && left[o] < left[o - 1]) { printf("left not monotone at %d of %d -> %d\n", o, in, out); return 1; }
    }
    return 0;
}

int main() {
    static const int pairs[][2] = { { 1, 1 }, { 1, 16384 }, { 16384, 1 }, { 16384, 16384 }, { 16384, 1537 }, { 1537, 16384 }, { 2, 5 }, { 5, 2 }, { 17, 16 },
                                    { 1066, 100 }, { 200, 19 }, { 1024, 32 }, { 1600, 100 }, { 16384, 512 }, { 16383, 16384 }, { 3, 16384 } };
    int tables = 0, refused = 0;
    for (const auto& p : pairs)
        for (int filter = 0; filter < 3; ++filter)
            for (int kind = 0; kind < 3; ++kind) {
                const int rc = check(p[0], p[1], filter, kind);
                if (rc == FLDR_RATE_E_ARG && scale_taps_count(p[0], p[1], filter) < 0) { ++refused; continue; }      // beyond the tap limit
                if (rc) { printf("%d -> %d filter %d kind %d: %d\n", p[0], p[1], filter, kind, rc); return 1; }
                ++tables;
            }
    // the limits themselves
    if (scale_taps_count(1066, 100, FLDR_SCALE_LANCZOS3) != 64 || scale_taps_count(1067, 100, FLDR_SCALE_LANCZOS3) >= 0 ||
        scale_taps_count(1024, 32, FLDR_SCALE_BILINEAR) != 64 || scale_taps_count(1600, 100, FLDR_SCALE_BICUBIC) != 64 ||
        scale_taps_count(0, 1, 0) >= 0 || scale_taps_count(16385, 1, 0) >= 0 || scale_taps_count(1, 16385, 0) >= 0 || scale_taps_count(1, 1, 3) >= 0) {
        printf("limits\n");
        return 1;
    }
    int32_t l;
    int16_t q[2];
    if (scale_taps(1, 1, 0, 3, &l, q) != FLDR_RATE_E_ARG || scale_taps(1, 1, 0, 0, nullptr, q) != FLDR_RATE_E_ARG || scale_taps(1, 1, 0, 0, &l, nullptr) != FLDR_RATE_E_ARG)
        return 1;
    printf("tables ok: %d built, %d refused at the tap limit\n", tables, refused);
    return 0;
}
