// libfldr_conform.so, shared between the host side (conform_host.hip) and the kernel (conform_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fldr_conform.h"

namespace fldr_conform_impl {

constexpr int CONFORM_THREADS = 256;   // lanes of a workgroup: 256 consecutive runs of one plane, row by row
constexpr int RUN_BYTES = 16;          // of an output row one lane owns: 16 samples at depth 8, 8 at depth 10

// the container of a side: layout x depth
enum { LAY_NV8 = 0,                    // NV12, bytes
       LAY_I8 = 1,                     // I420, bytes
       LAY_P010 = 2,                   // NV12, the value in the high 10 bits of a word
       LAY_LOW10 = 3 };                // I420, the value in the low 10 bits of a word

// One conform.  A luma run is RUN_BYTES of a luma row; a chroma run is RUN_BYTES of every chroma plane of the output at the same columns:
// 16 / 8 columns of both planes of I420, 8 / 4 columns of NV12's one.
struct ConformArgs {
    const uint8_t* src[3];
    uint8_t* dst[3];
    int64_t pitch_src[3], pitch_dst[3];
    int in_H, in_W, out_H, out_W;
    int dst_x, dst_y;
    int kyy, kyu, kyv, kuu, kuv, kvu, kvv;
    int yo_s, cc_s, yo_d, cc_d;
    int dither;
    uint32_t luma_runs, chroma_runs;   // of a row
    uint32_t luma_blocks, blocks;      // workgroups of the luma plane; of all planes
};

// lay_in, lay_out: LAY_* numbers; matrix: the matrices differ (kyu, kyv, kuv, kvu are zero otherwise and the luma pass reads no chroma).
// One launch on `stream`; the arguments have been checked.
int conform(const ConformArgs& a, int lay_in, int lay_out, bool matrix, hipStream_t stream);

}  // namespace fldr_conform_impl
