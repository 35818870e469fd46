// libfldr_cadence.so, shared between the host side (cadence_host.hip) and the kernels (cadence_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../rate/tile_reduce_device.h"
#include "fldr_cadence.h"

namespace fldr_cadence_impl {
using namespace fldr_tile_reduce;

// The repeat state (FLDR_REPEAT_STATE_BYTES of device memory) in lines of 64 bytes: line 0 begins with the result the caller reads,
// lines 1 .. SLOTS are the kernels' accumulator slots; workgroup b adds to slot 1 + b % SLOTS (../rate/tile_reduce_device.h).
constexpr int STATE_SLOT_BYTES = 64;
constexpr int SLOT_SAD_OFFSET = 0;         // uint64: the sum of the tile sums of the slot's workgroups
constexpr int SLOT_KEY_OFFSET = 8;         // uint64: max over their tiles of (tile_sad << 32) | (0xffffffff - index)
constexpr int SLOT_MOVING_OFFSET = 16;     // uint32: their tiles with tile_sad >= tile_sad_min

// zero `state`, reduce every tile of the two luma planes, write the result: three launches on `stream`
int repeat_measure(const void* y0, int64_t pitch0, const void* y1, int64_t pitch1, int H, int W, int mode, int tile_sad_min, void* state,
                   hipStream_t stream);

}  // namespace fldr_cadence_impl
