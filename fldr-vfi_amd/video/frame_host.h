// The host side of the frame contract of include/fldr_video.h (what a valid format and a valid frame are, how large a plane is) and the
// plumbing of a stream object (fldr_video_session, fldr_rate): a device, a stream, one device block, one pinned block, packed frames in
// them.  Included by video_host.hip, ../chroma/chroma_host.hip, ../pack10/pack10_host.hip and ../rgb/rgb_host.hip (through
// yuv_stream_host.h), by the shutter and light libraries' host files and, through ../rate/rate_plan.h, by the rate, pipe, cadence, field,
// pulldown and interlace libraries': each refuses exactly the frames libfldr_video.so refuses because all compile this text (the chroma, pack10
// and rgb libraries with their own FrameRules, below).  Everything is in the unnamed namespace: nothing here becomes a symbol of any
// library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "fldr_video.h"

namespace {

constexpr int64_t ALIGN = 256;
int64_t align_up(int64_t v) { return (v + ALIGN - 1) / ALIGN * ALIGN; }

#define CK(x) do { const int rc_ = (x); if (rc_) return rc_; } while (0)

// ---- formats and frames -----------------------------------------------------------------------------------------------------------
int planes_of(int layout) { return layout == FLDR_VIDEO_NV12 ? 2 : 3; }

template <class Format> bool deep(const Format& f) { return f.depth == 10; }       // 16-bit words (depth 0 is an alias of 8)

int check_format(const fldr_video_format& f) {
    if ((unsigned)f.layout > 1u || (unsigned)f.matrix > 1u || (unsigned)f.range > 1u) return FLDR_VIDEO_E_FORMAT;
    if (f.depth != 0 && f.depth != 8 && f.depth != 10) return FLDR_VIDEO_E_FORMAT;
    for (int i = 0; i < 4; ++i) if (f.reserved[i]) return FLDR_VIDEO_E_FORMAT;
    return 0;
}

// bytes per row of plane p of a frame of width W
int64_t row_bytes(const fldr_video_format& f, int p, int W) {
    const int64_t cw = (W + 1) / 2, b = deep(f) ? 2 : 1;
    return b * (p == 0 ? W : (f.layout == FLDR_VIDEO_NV12 ? 2 * cw : cw));
}

int rows_of(int p, int H) { return p == 0 ? H : (H + 1) / 2; }

// The functions below are written once for every format struct (a `depth` word: 10 = 16-bit samples, and frames of plane[] / pitch[]).
// A library states its own rules in a FrameRules<Format>, specialised before the first call that uses it: the frame type, its E_PLANE /
// E_PITCH codes, the planes of a format, the bytes per row and the rows of plane p, and the format's address unit (the bytes of which
// every plane pointer and pitch must be a multiple beyond the sample size: 4 for a container of 32-bit words, 0 for none).  These are
// fldr_video.h's (4:2:0); the chroma, pack10 and rgb libraries' host files have theirs.
template <class Format> struct FrameRules;
template <> struct FrameRules<fldr_video_format> {
    using Frame = fldr_video_frame;
    static constexpr int E_PLANE = FLDR_VIDEO_E_PLANE, E_PITCH = FLDR_VIDEO_E_PITCH;
    static int planes(const fldr_video_format& f) { return planes_of(f.layout); }
    static int64_t row_bytes(const fldr_video_format& f, int p, int W) { return ::row_bytes(f, p, W); }
    static int rows(const fldr_video_format&, int p, int H) { return rows_of(p, H); }
    static int unit(const fldr_video_format&) { return 0; }
};
template <class Format> using FrameOf = typename FrameRules<Format>::Frame;

// Every plane and every pitch by the sample size first, then every plane and every pitch by the address unit: a frame with two faults
// gets the code of the earlier of these four passes.
template <class Format> int check_frame(const FrameOf<Format>& fr, const Format& f, int W) {
    using R = FrameRules<Format>;
    const bool words = f.depth == 10;
    const int np = R::planes(f);
    for (int p = 0; p < np; ++p) if (!fr.plane[p] || (words && ((uintptr_t)fr.plane[p] & 1))) return R::E_PLANE;
    for (int p = 0; p < np; ++p)
        if (fr.pitch[p] < R::row_bytes(f, p, W) || (words && (fr.pitch[p] & 1))) return R::E_PITCH;
    const uintptr_t unit = (uintptr_t)R::unit(f);
    if (unit) {
        for (int p = 0; p < np; ++p) if ((uintptr_t)fr.plane[p] % unit) return R::E_PLANE;
        for (int p = 0; p < np; ++p) if ((uintptr_t)fr.pitch[p] % unit) return R::E_PITCH;
    }
    return 0;
}

// ---- packed frames ----------------------------------------------------------------------------------------------------------------
// packed planes of one frame (pitch = row bytes) starting at `base`
template <class Format> FrameOf<Format> packed(uint8_t* base, const Format& fmt, int H, int W) {
    using R = FrameRules<Format>;
    FrameOf<Format> f;
    memset(&f, 0, sizeof(f));
    int64_t off = 0;
    for (int p = 0; p < R::planes(fmt); ++p) {
        f.plane[p] = base + off;
        f.pitch[p] = R::row_bytes(fmt, p, W);
        off += f.pitch[p] * R::rows(fmt, p, H);
    }
    return f;
}

template <class Format> int64_t packed_bytes(const Format& fmt, int H, int W) {
    using R = FrameRules<Format>;
    int64_t n = 0;
    for (int p = 0; p < R::planes(fmt); ++p) n += R::row_bytes(fmt, p, W) * R::rows(fmt, p, H);
    return n;
}

// A 4:2:0 frame whose pitches are the row bytes rounded up to 16, so that every plane and pitch is 16-byte aligned whatever W is and a
// kernel over it runs its 16-byte form (the I420 chroma rows of a 720-wide frame are 360 bytes): the frames the deinterlacing and
// interlacing streams hold on the device and in pinned memory.
constexpr int64_t SLOT_PITCH = 16;

int64_t padded_pitch(const fldr_video_format& f, int p, int W) { return (row_bytes(f, p, W) + SLOT_PITCH - 1) / SLOT_PITCH * SLOT_PITCH; }

fldr_video_frame padded(uint8_t* base, const fldr_video_format& f, int H, int W) {
    fldr_video_frame fr;
    memset(&fr, 0, sizeof(fr));
    int64_t off = 0;
    for (int p = 0; p < planes_of(f.layout); ++p) {
        fr.plane[p] = base + off;
        fr.pitch[p] = padded_pitch(f, p, W);
        off += fr.pitch[p] * rows_of(p, H);
    }
    return fr;
}

int64_t padded_bytes(const fldr_video_format& f, int H, int W) {
    int64_t n = 0;
    for (int p = 0; p < planes_of(f.layout); ++p) n += padded_pitch(f, p, W) * rows_of(p, H);
    return n;
}

// the bytes a plane of a 4:2:0 frame occupies: [lo, hi)
void extent(const fldr_video_frame& f, const fldr_video_format& fmt, int p, int H, int W, uintptr_t& lo, uintptr_t& hi) {
    lo = (uintptr_t)f.plane[p];
    hi = lo + (uintptr_t)(f.pitch[p] * (rows_of(p, H) - 1) + row_bytes(fmt, p, W));
}

// any plane of `out` shares a byte with any plane of `in`
bool overlaps(const fldr_video_frame& out, const fldr_video_frame& in, const fldr_video_format& fmt, int H, int W) {
    for (int p = 0; p < planes_of(fmt.layout); ++p)
        for (int q = 0; q < planes_of(fmt.layout); ++q) {
            uintptr_t a0, a1, b0, b1;
            extent(out, fmt, p, H, W, a0, a1);
            extent(in, fmt, q, H, W, b0, b1);
            if (a0 < b1 && b0 < a1) return true;
        }
    return false;
}

// rows of every plane from `src` (any pitches) to `dst` (any pitches), on the host
template <class Format> void copy_planes(const FrameOf<Format>& dst, const FrameOf<Format>& src, const Format& fmt, int H, int W) {
    using R = FrameRules<Format>;
    for (int p = 0; p < R::planes(fmt); ++p) {
        const int64_t rb = R::row_bytes(fmt, p, W), n = R::rows(fmt, p, H);
        for (int64_t r = 0; r < n; ++r)
            memcpy((uint8_t*)dst.plane[p] + r * dst.pitch[p], (const uint8_t*)src.plane[p] + r * src.pitch[p], (size_t)rb);
    }
}

// ---- a device, a stream on it, one device block, one pinned block -------------------------------------------------------------------
struct DeviceGuard {                                      // make `dev` current, restore the caller's device on exit
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev && hipSetDevice(dev) != hipSuccess) ok = false;
    }
    ~DeviceGuard() { if (prev >= 0) { int cur = -1; if (hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev); } }
};

struct StreamMem {
    int device = -1;
    hipStream_t stream = nullptr;      // non-blocking
    uint8_t* dev = nullptr;
    uint8_t* pinned = nullptr;
};

void close_stream_mem(StreamMem& m) {
    DeviceGuard g(m.device);
    if (m.stream) (void)hipStreamDestroy(m.stream);
    if (m.dev) (void)hipFree(m.dev);
    if (m.pinned) (void)hipHostFree(m.pinned);
    (void)hipGetLastError();
    m = StreamMem();
}

// all of it or nothing: false (no such device, out of memory) leaves `m` empty
bool open_stream_mem(StreamMem& m, int device, int64_t dev_bytes, int64_t pinned_bytes) {
    m = StreamMem();
    m.device = device;
    DeviceGuard g(device);
    if (g.ok && hipMalloc((void**)&m.dev, (size_t)dev_bytes) == hipSuccess &&
        hipHostMalloc((void**)&m.pinned, (size_t)pinned_bytes, hipHostMallocDefault) == hipSuccess &&
        hipStreamCreateWithFlags(&m.stream, hipStreamNonBlocking) == hipSuccess)
        return true;
    close_stream_mem(m);
    return false;
}

// one host frame (any pitches) -> packed in `pinned_slot` -> enqueued to `dev_slot`; the pinned copy stays valid for the caller
template <class Format>
hipError_t upload_frame(const StreamMem& m, uint8_t* dev_slot, uint8_t* pinned_slot, int64_t slot_bytes, const FrameOf<Format>& src,
                        const Format& fmt, int H, int W) {
    copy_planes(packed(pinned_slot, fmt, H, W), src, fmt, H, W);
    return hipMemcpyAsync(dev_slot, pinned_slot, (size_t)slot_bytes, hipMemcpyHostToDevice, m.stream);
}

// one packed frame in the pinned block -> the caller's planes
template <class Format> void unpack_frame(const FrameOf<Format>& dst, uint8_t* pinned_slot, const Format& fmt, int H, int W) {
    copy_planes(dst, packed(pinned_slot, fmt, H, W), fmt, H, W);
}

}  // namespace
