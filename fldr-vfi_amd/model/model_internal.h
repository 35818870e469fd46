// Internals shared by the two translation units of libfldr_model.so (hidden: -fvisibility=hidden + model/exports.map).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fldr_model.h"

#define MI_MAX_LEVELS 7          // level 0 + factors 2 ... 64 from one 64 x 64 tile (as fldr_ingest_pyramid_u8)

namespace fldr_model_impl {
int ingest_interleaved_pyramid(const uint8_t* const frame[2], const int64_t pitch[2], int rgb, float* const* levels, int n_levels,
                               int H, int W, int Hp, int Wp, hipStream_t stream);
int planar_to_interleaved(const uint8_t* src, uint8_t* dst, int64_t pitch, int rgb, int H, int W, hipStream_t stream);
}  // namespace fldr_model_impl
