// The host side of a luma tile measure (fldr_repeat_measure, fldr_pulldown_measure, fldr_probe_measure), written once: which frame sizes
// the tile reduce of tile_reduce_device.h takes, the order in which several frames are checked, the check of the state, the luma planes
// a measure call begins with, and the wait that follows a failed enqueue.  Included by ../cadence/cadence_host.hip and
// ../pulldown/pulldown_host.hip (through cycle_stream_host.h), by ../probe/probe_host.hip and, for check_frames, by
// ../interlace/interlace_host.hip (../field/field_host.hip checks its frames one by one and does not include it); it includes
// ../video/frame_host.h only, so a library that includes it calls no fldr_* function it did not call before.  Everything is in the
// unnamed namespace, as there.
#pragma once
#include "../video/frame_host.h"

namespace {

// rows and columns rounded up to whole tiles of T x T stay inside 32 bits, and the key holds the tile index in 31 bits
bool tiles_ok(int H, int W, int64_t T) {
    if (H < 1 || W < 1 || H > 0x7fffffff - T || W > 0x7fffffff - T) return false;
    return ((int64_t)W + T - 1) / T * (((int64_t)H + T - 1) / T) <= 0x7fffffffll;
}

// planes, then pitches, of the frames given (null entries are skipped), in order: the video library's codes
int check_frames(const fldr_video_frame* const* fr, int n, const fldr_video_format& fmt, int W) {
    const bool words = deep(fmt);
    for (int f = 0; f < n; ++f) {
        if (!fr[f]) continue;
        for (int p = 0; p < planes_of(fmt.layout); ++p)
            if (!fr[f]->plane[p] || (words && ((uintptr_t)fr[f]->plane[p] & 1))) return FLDR_VIDEO_E_PLANE;
    }
    for (int f = 0; f < n; ++f) if (fr[f]) CK(check_frame(*fr[f], fmt, W));
    return 0;
}

// the measure state: device memory the caller gives, ALIGN-aligned; `code` is the library's answer to a missing or misaligned one
int check_state(const void* state, int code) { return !state || ((uintptr_t)state & (ALIGN - 1)) ? code : 0; }

// what a MeasureCall begins with: plane 0 of cur, and of prev and next where they are given (null, pitch 0: not measured)
template <class Call> void fill_luma(Call& c, const fldr_video_frame* cur, const fldr_video_frame* prev, const fldr_video_frame* next) {
    c.cur = cur->plane[0]; c.pitch_cur = cur->pitch[0];
    c.prev = prev ? prev->plane[0] : nullptr; c.pitch_prev = prev ? prev->pitch[0] : 0;
    c.next = next ? next->plane[0] : nullptr; c.pitch_next = next ? next->pitch[0] : 0;
}

// after a failed enqueue, and before a reset: nothing enqueued may still write the pinned block, and the error is not left for the caller
void drain(StreamMem& sm) {
    (void)hipStreamSynchronize(sm.stream);
    (void)hipGetLastError();
}

}  // namespace
