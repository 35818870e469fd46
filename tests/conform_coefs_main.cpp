// The table builder of libfldr_conform.so (fldr-vfi_amd/conform/conform_coefs.h) as a stand-alone host program, for the host sanitizers:
//   g++ -std=c++17 -fsanitize=address,undefined -Iinclude -Ifldr-vfi_amd/conform tests/conform_coefs_main.cpp && ./a.out
// It builds the table of every (matrix, range, depth) pair into a buffer of exactly seven words (so that a write past it is seen), checks
// the entries that are exact by definition, the issue's worked table, and that the largest sum the kernel can form fits int32.
// tests/test_conform_cpu.py builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "conform_coefs.h"

using namespace fldr_conform_impl;

static fldr_video_format format_of(int matrix, int range, int depth) {
    fldr_video_format f = {};
    f.layout = FLDR_VIDEO_NV12;
    f.matrix = matrix; f.range = range; f.depth = depth;
    return f;
}

int main() {
    static const int depths[3] = { 0, 8, 10 };                          // 0 is an alias of 8
    int tables = 0;
    long long worst = 0;
    for (int a = 0; a < 12; ++a)
        for (int b = 0; b < 12; ++b) {
            const fldr_video_format s = format_of(a & 1, (a >> 1) & 1, depths[a >> 2]), d = format_of(b & 1, (b >> 1) & 1, depths[b >> 2]);
            std::vector<int32_t> k(7);
            conform_coefs(s, d, k.data());
            const ConformSide ss = conform_side(s), dd = conform_side(d);
            if (s.matrix == d.matrix && (k[FLDR_CONFORM_KYU] || k[FLDR_CONFORM_KYV] || k[FLDR_CONFORM_KUV] || k[FLDR_CONFORM_KVU])) {
                printf("equal matrices with a cross term: %d -> %d\n", a, b);
                return 1;
            }
            if (s.matrix == d.matrix && ss.ys == dd.ys && ss.cs == dd.cs &&
                (k[FLDR_CONFORM_KYY] != 16384 || k[FLDR_CONFORM_KUU] != 16384 || k[FLDR_CONFORM_KVV] != 16384)) {
                printf("equal formats without the unit: %d -> %d\n", a, b);
                return 1;
            }
            const long long cmax = 8ll * (ss.mx - ss.cc > ss.cc ? ss.mx - ss.cc : ss.cc), ymax = ss.mx - ss.yo > ss.yo ? ss.mx - ss.yo : ss.yo;
            const long long sum = 8ll * llabs(k[FLDR_CONFORM_KYY]) * ymax + (llabs(k[FLDR_CONFORM_KYU]) + llabs(k[FLDR_CONFORM_KYV])) * cmax +
                                  (1ll << 17) + ((long long)dd.yo << 17);
            if (sum > worst) worst = sum;
            ++tables;
        }
    if (worst >= (1ll << 31)) { printf("a luma sum of %lld does not fit int32\n", worst); return 1; }
    int32_t k[7];
    conform_coefs(format_of(FLDR_VIDEO_BT601, FLDR_VIDEO_LIMITED, 8), format_of(FLDR_VIDEO_BT709, FLDR_VIDEO_LIMITED, 8), k);
    static const int32_t want[7] = { 16384, -1893, -3407, 16689, 1878, 1230, 16799 };
    for (int i = 0; i < 7; ++i)
        if (k[i] != want[i]) { printf("601 -> 709: word %d is %d, not %d\n", i, k[i], want[i]); return 1; }
    printf("coefs ok: %d tables, worst luma sum %lld\n", tables, worst);
    return 0;
}
