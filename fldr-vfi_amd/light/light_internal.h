// libfldr_light.so, shared between the host side (light_host.hip) and the kernels (light_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fldr_light.h"

namespace fldr_light_impl {

constexpr int MAX_FRAMES = FLDR_SHUTTER_LAUNCH_FRAMES;
constexpr int MAX_CODES = 1024;

// The kernels work on planar BGR code values: `count` = 3 H W samples in a row (bytes at depth 8, 16-bit words at depth 10), as the
// video library's converters write and read them.  The accumulator is one uint32 per sample in the same order.
struct Sources {
    const void* codes[MAX_FRAMES];     // `count` samples each
    uint32_t weight[MAX_FRAMES];
    int n;
};

// the device side of a curve: lin[0 .. codes), then mid[0 .. codes) (mid[0] unused)
struct Tables {
    const uint32_t* lin;
    const uint32_t* mid;
};

// vec: every source address is 16-byte aligned.  acc and out are always 256-byte aligned.
int launch_accumulate(bool deep, int64_t count, const Tables& t, const Sources& src, bool first, uint32_t* acc, bool vec, hipStream_t stream);
int launch_resolve(bool deep, int64_t count, const Tables& t, const uint32_t* acc, uint32_t total, void* out, hipStream_t stream);
int launch_mix(bool deep, int64_t count, const Tables& t, const Sources& src, uint32_t total, void* out, bool vec, hipStream_t stream);

}  // namespace fldr_light_impl
