// libfldr_field.so, shared between the host side (field_host.hip) and the kernel (field_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../rate/luma8_device.h"
#include "../video/weave_walk_device.h"
#include "fldr_field.h"

namespace fldr_field_impl {
using fldr_luma8::luma_mode;          // the sample form of a format: a fldr_sample16::FORM_* number

// One plane of a weave: the sources and what ../video/weave_walk_device.h says every plane carries (a work item is one 16-byte column
// group of one own-parity row).  `comp` is the distance, in samples, between neighbouring samples of one component: 2 in the
// interleaved NV12 chroma plane, 1 elsewhere.
struct WeavePlane {
    const uint8_t* cur;
    const uint8_t* prev;
    const uint8_t* next;
    const uint8_t* temporal;
    uint8_t* out;
    int64_t pitch_cur, pitch_prev, pitch_next, pitch_temporal, pitch_out;
    int64_t row_bytes;
    int rows;
    int comp;                          // 1 / 2
    int vec;
    uint32_t groups, groups_magic, first;
};

struct WeaveArgs {
    WeavePlane pl[3];
    int planes;
    int parity;
    int intra;                         // the mode of the call
    const uint32_t* intra_if;          // may be null
    int still, slack;
    uint32_t total;                    // work items of all planes
};

// form: a fldr_sample16::FORM_* number.  One launch on `stream`; the arguments have been checked.
int weave(const WeaveArgs& a, int form, hipStream_t stream);

}  // namespace fldr_field_impl
