// libfldr_scale.so, shared between the host side (scale_host.hip) and the kernel (scale_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../rate/luma8_device.h"
#include "fldr_scale.h"

namespace fldr_scale_impl {
using fldr_luma8::luma_mode;          // the sample form of a format: a fldr_sample16::FORM_* number

constexpr int SCALE_THREADS = 256;
constexpr int TILE_GROUPS = 16;        // 16-byte groups of an output row one workgroup owns: 256 samples at depth 8, 128 at depth 10
constexpr int TILE_ROWS_MAX = 16;      // ... and at most this many output rows: one group of one row per thread
constexpr int LDS_LIMIT = 65536;
constexpr int STAGE_ROWS_BYTE = 4;     // source rows of a staged chunk at depth 8; twice that at depth 10, where a tile row is half the threads
constexpr int STAGE_LIMIT = 32768;     // a staged chunk may take this much of the LDS: a tile of one output row (at most 32 KB of m) still fits beside it

// One plane of a scale.  A row of the plane is `out_w` samples; with cshift = 1 (the interleaved chroma plane of NV12) sample x is
// component x & 1 of chroma column x >> 1, and the horizontal table is indexed by the column.
struct ScalePlane {
    const uint8_t* src;
    uint8_t* dst;
    int64_t pitch_src, pitch_dst;
    const int32_t* left_x;             // device tables: one word per output column, nx coefficients per output column, ...
    const int16_t* coef_x;
    const int32_t* left_y;
    const int16_t* coef_y;
    int in_cols, in_rows;              // source columns (per component) and rows: what the indices clamp to
    int out_w, out_rows;               // output samples per row (all components) and rows
    int cshift;
    int tile_w, tile_h;                // tile_w: TILE_GROUPS groups in samples
    int vec;                           // dst and pitch_dst are multiples of 16
    int stage_span;                    // 0: the horizontal pass loads from global memory; else the samples of a staged source row in LDS
    uint32_t tiles_x, first;           // tiles across; the first workgroup of the plane
};

struct ScaleArgs {
    ScalePlane pl[3];
    int planes;
    int nx, ny;
    int stage_at;                      // where the staged chunk begins in LDS, in int16 behind the intermediate
    uint32_t total;                    // workgroups of all planes
};

// form: a fldr_sample16::FORM_* number.  One launch on `stream` with lds_bytes of dynamic LDS; the arguments have been checked.
int scale(const ScaleArgs& a, int form, int lds_bytes, hipStream_t stream);

}  // namespace fldr_scale_impl
