// libfldr_interlace.so, shared between the host side (interlace_host.hip) and the kernel (interlace_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../rate/luma8_device.h"
#include "../video/weave_walk_device.h"
#include "fldr_interlace.h"

namespace fldr_interlace_impl {
using fldr_luma8::luma_mode;          // the sample form of a format: a fldr_sample16::FORM_* number

// One plane of a weave: the sources and what ../video/weave_walk_device.h says every plane carries (a work item is one 16-byte column
// group of one output row).
struct WeavePlane {
    const uint8_t* even;               // the source of the rows y % 2 == 0; null: those rows are not written
    const uint8_t* odd;                // of the rows y % 2 == 1
    uint8_t* out;
    int64_t pitch_even, pitch_odd, pitch_out;
    int64_t row_bytes;
    int rows;
    int vec;
    uint32_t groups, groups_magic, first;
};

struct WeaveArgs {
    WeavePlane pl[3];
    int planes;
    int start, step;                   // output row of a plane's item row i: start + step x i (0, 1: both parities; q, 2: parity q alone)
    uint32_t total;                    // work items of all planes
};

// form: a fldr_sample16::FORM_* number; filter: FLDR_INTERLACE_NONE / _LINEAR / _COMPLEX.  One launch on `stream`; the arguments have
// been checked.
int weave(const WeaveArgs& a, int form, int filter, hipStream_t stream);

}  // namespace fldr_interlace_impl
