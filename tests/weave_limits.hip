// weave_limits field|interlace nv12|i420 8|10 H W -> "accept" or "refuse": whether the weave of that library takes an H x W frame, by the
// fill of its planes' walks (fldr-vfi_amd/video/weave_walk_host.h) with the two row counts the library passes per plane — field_host.hip:
// the own rows, twice; interlace_host.hip with both sources given: all rows, twice.  No HIP call is made: tests/test_weave_limits_cpu.py
// builds and runs this without a GPU, on both sides of every limit (an accepted call of the library itself would launch a kernel).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../fldr-vfi_amd/video/weave_walk_host.h"

struct Walk {                          // what fill_walk fills: weave_walk_device.h
    uint8_t* out;
    int64_t pitch_out, row_bytes;
    int rows, vec;
    uint32_t groups, groups_magic, first;
};

int main(int argc, char** argv) {
    if (argc != 6) return 2;
    const bool field = !strcmp(argv[1], "field");
    fldr_video_format f;
    memset(&f, 0, sizeof(f));
    f.layout = !strcmp(argv[2], "nv12") ? FLDR_VIDEO_NV12 : FLDR_VIDEO_I420;
    f.depth = atoi(argv[3]);
    const int H = atoi(argv[4]), W = atoi(argv[5]);
    if ((!field && strcmp(argv[1], "interlace")) || (f.layout == FLDR_VIDEO_I420 && strcmp(argv[2], "i420")) || check_format(f) || !size_ok(H) || W < 1)
        return 2;
    fldr_video_frame out;
    memset(&out, 0, sizeof(out));
    int64_t total = 0;
    bool ok = true;
    for (int p = 0; p < planes_of(f.layout) && ok; ++p) {
        Walk q;
        const int64_t rows = rows_of(p, H);
        ok = field ? fill_walk(q, f, p, H, W, out, rows / 2, rows / 2, total) : fill_walk(q, f, p, H, W, out, rows, rows, total);
    }
    puts(ok ? "accept" : "refuse");
    return 0;
}
