// libfldr_shutter.so, shared between the host side (shutter_host.hip) and the kernels (shutter_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../video/sample16_device.h"
#include "fldr_shutter.h"

namespace fldr_shutter_impl {

// how the value sits in a sample
enum { S_BYTE = fldr_sample16::FORM_BYTE,        // depth 8: the byte
       S_P010 = fldr_sample16::FORM_P010,        // word >> 6, written as v << 6
       S_LOW10 = fldr_sample16::FORM_LOW10 };    // word & 0x3ff, written as v

constexpr int MAX_FRAMES = FLDR_SHUTTER_LAUNCH_FRAMES;

// A frame as the kernels walk it: plane by plane (blockIdx.y), row by row, in groups of 16 bytes.  The accumulator holds the whole
// groups of every plane first (group g of a plane at 16 / bytes-per-sample uint32 from its `acc_full`, so every group is a whole
// number of aligned uint4), then the samples of the rows' partial last groups (`acc_tail`), row after row.
struct Geometry {
    int64_t row_bytes[3];
    int64_t acc_full[3];               // in uint32 units
    int64_t acc_tail[3];
    uint32_t chunks[3];                // groups per row, the partial last one included
    uint32_t full[3];                  // whole groups per row
    uint32_t items[3];                 // rows * chunks
    int np;
    int mode;
    int64_t samples;                   // of the packed frame
};

struct Sources {
    const uint8_t* plane[MAX_FRAMES][3];
    int64_t pitch[MAX_FRAMES][3];
    uint32_t weight[MAX_FRAMES];
    int n;
};

struct Target {
    uint8_t* plane[3];
    int64_t pitch[3];
    uint32_t total, mul, shift, maxv;
};

// false when the frame has more 16-byte groups in a plane than the kernels count in 32 bits
bool geometry(int H, int W, const fldr_video_format& fmt, Geometry& g);

// x / (2 total) for x <= 2047 total as ((uint64_t)x * mul >> 32) >> shift
void reciprocal(uint32_t total, uint32_t& mul, uint32_t& shift);

// vec: every plane address and pitch of the frames involved is 16-byte aligned
int launch_accumulate(const Geometry& g, const Sources& src, bool first, uint32_t* acc, bool vec, hipStream_t stream);
int launch_resolve(const Geometry& g, const uint32_t* acc, const Target& dst, bool vec, hipStream_t stream);
int launch_mix(const Geometry& g, const Sources& src, const Target& dst, bool vec, hipStream_t stream);

}  // namespace fldr_shutter_impl
