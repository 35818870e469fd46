// The host side of the frame contract of include/fldr_video.h (what a valid format and a valid frame are, how large a plane is) and the
// plumbing of a stream object (fldr_video_session, fldr_rate): a device, a stream, one device block, one pinned block, packed or padded
// frames in them, and the stream over padded frames of the field and interlace libraries (PaddedStream).  Included by video_host.hip,
// ../chroma/chroma_host.hip, ../pack10/pack10_host.hip and ../rgb/rgb_host.hip (through yuv_stream_host.h), by the shutter and light
// libraries' host files, through ../rate/rate_plan.h by the rate, pipe, cadence, field, pulldown and interlace libraries', through
// ../rate/tile_measure_host.h by the probe library's, and by weave_walk_host.h: each refuses exactly the frames libfldr_video.so refuses
// because all compile this text (the chroma, pack10 and rgb libraries with their own FrameRules, below).  Everything is in the unnamed
// namespace: nothing here becomes a symbol of any library.
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
    const int64_t cw = ((int64_t)W + 1) / 2, b = deep(f) ? 2 : 1;          // W + 1 is no int at W = 2^31 - 1
    return b * (p == 0 ? W : (f.layout == FLDR_VIDEO_NV12 ? 2 * cw : cw));
}

int rows_of(int p, int H) { return p == 0 ? H : (int)(((int64_t)H + 1) / 2); }

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

// ---- frames in a block ------------------------------------------------------------------------------------------------------------
// The planes of one frame one after the other, each pitch the row bytes rounded up to `unit`.  PACKED_PITCH: pitch = row bytes, the
// frames most stream objects hold.  SLOT_PITCH: every plane and pitch is 16-byte aligned whatever W is, so that a kernel over the frame
// runs its 16-byte form (the I420 chroma rows of a 720-wide frame are 360 bytes): the 4:2:0 frames the deinterlacing and interlacing
// streams hold on the device and in pinned memory.
constexpr int64_t PACKED_PITCH = 1, SLOT_PITCH = 16;

template <class Format> int64_t pitch_of(const Format& fmt, int p, int W, int64_t unit) {
    return (FrameRules<Format>::row_bytes(fmt, p, W) + unit - 1) / unit * unit;
}

// the frame of that layout starting at `base`
template <class Format> FrameOf<Format> laid_out(uint8_t* base, const Format& fmt, int H, int W, int64_t unit) {
    using R = FrameRules<Format>;
    FrameOf<Format> f;
    memset(&f, 0, sizeof(f));
    int64_t off = 0;
    for (int p = 0; p < R::planes(fmt); ++p) {
        f.plane[p] = base + off;
        f.pitch[p] = pitch_of(fmt, p, W, unit);
        off += f.pitch[p] * R::rows(fmt, p, H);
    }
    return f;
}

template <class Format> int64_t laid_out_bytes(const Format& fmt, int H, int W, int64_t unit) {
    using R = FrameRules<Format>;
    int64_t n = 0;
    for (int p = 0; p < R::planes(fmt); ++p) n += pitch_of(fmt, p, W, unit) * R::rows(fmt, p, H);
    return n;
}

template <class Format> FrameOf<Format> packed(uint8_t* base, const Format& fmt, int H, int W) { return laid_out(base, fmt, H, W, PACKED_PITCH); }
template <class Format> int64_t packed_bytes(const Format& fmt, int H, int W) { return laid_out_bytes(fmt, H, W, PACKED_PITCH); }
fldr_video_frame padded(uint8_t* base, const fldr_video_format& f, int H, int W) { return laid_out(base, f, H, W, SLOT_PITCH); }
int64_t padded_bytes(const fldr_video_format& f, int H, int W) { return laid_out_bytes(f, H, W, SLOT_PITCH); }

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

// `device` (not negative) is one of the devices there are
bool device_exists(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && device < ndev) return true;
    (void)hipGetLastError();
    return false;
}

// one host frame (any pitches) -> laid out by `unit` in `pinned_slot` -> enqueued to `dev_slot`, gap bytes and all (they are never read);
// the pinned copy stays valid for the caller
template <class Format>
hipError_t upload_frame(const StreamMem& m, uint8_t* dev_slot, uint8_t* pinned_slot, int64_t slot_bytes, const FrameOf<Format>& src,
                        const Format& fmt, int H, int W, int64_t unit = PACKED_PITCH) {
    copy_planes(laid_out(pinned_slot, fmt, H, W, unit), src, fmt, H, W);
    return hipMemcpyAsync(dev_slot, pinned_slot, (size_t)slot_bytes, hipMemcpyHostToDevice, m.stream);
}

// one frame laid out by `unit` in the pinned block -> the caller's planes
template <class Format> void unpack_frame(const FrameOf<Format>& dst, uint8_t* pinned_slot, const Format& fmt, int H, int W, int64_t unit = PACKED_PITCH) {
    copy_planes(dst, laid_out(pinned_slot, fmt, H, W, unit), fmt, H, W);
}

// ---- a synchronous stream over padded 4:2:0 frames -----------------------------------------------------------------------------------
// What the deinterlacing stream (woven frames in, progressive frames out) and the interlacing stream (the reverse) share: the two device
// slots the input frames alternate in, one pinned input frame, the pinned output frames, and the two ends of a call — the upload of the
// pushed frame; the downloads, the wait and the hand-out.  Which frames are computed from the slots, where they lie on the device and
// what is reported stay with the library.
struct PaddedStream {
    StreamMem sm;
    fldr_video_format format;
    int H, W;
    int64_t frame_bytes;               // of a padded() frame, aligned up
    uint8_t* slot[2];                  // device: frame n lives in slot n & 1
    uint8_t* dev_rest;                 // device: what follows the slots, the library's
    uint8_t* in_host;                  // pinned: the frame being pushed
    uint8_t* out_host;                 // pinned: the output frames of a call, frame_bytes apart; behind them, the library's
};

// the device block: the two slots, dev_frames more frames and dev_rest bytes; the pinned block: the input frame, out_frames and
// host_rest bytes.  All of it or nothing, as open_stream_mem.
bool open_padded_stream(PaddedStream& s, int device, const fldr_video_format& f, int H, int W, int64_t dev_frames, int64_t dev_rest,
                        int64_t out_frames, int64_t host_rest) {
    s.format = f; s.H = H; s.W = W;
    s.frame_bytes = align_up(padded_bytes(f, H, W));
    if (!open_stream_mem(s.sm, device, (2 + dev_frames) * s.frame_bytes + dev_rest, (1 + out_frames) * s.frame_bytes + host_rest)) return false;
    s.slot[0] = s.sm.dev;
    s.slot[1] = s.slot[0] + s.frame_bytes;
    s.dev_rest = s.slot[1] + s.frame_bytes;
    s.in_host = s.sm.pinned;
    s.out_host = s.in_host + s.frame_bytes;
    return true;
}

fldr_video_frame padded_at(const PaddedStream& s, uint8_t* base) { return padded(base, s.format, s.H, s.W); }

// frame n of the stream: the caller's planes -> the pinned input frame -> enqueued to slot n & 1
hipError_t upload_input(const PaddedStream& s, int64_t n, const fldr_video_frame& frame) {
    return upload_frame(s.sm, s.slot[n & 1], s.in_host, s.frame_bytes, frame, s.format, s.H, s.W, SLOT_PITCH);
}

// the frames a call will hand out: `e_arg` without them, the frame rules' codes for a bad one
int check_outs(const PaddedStream& s, const fldr_video_frame* host_outs, int count, int e_arg) {
    if (!count) return 0;
    if (!host_outs) return e_arg;
    for (int k = 0; k < count; ++k) CK(check_frame(host_outs[k], s.format, s.W));
    return 0;
}

// The end of a call whose enqueues came to `rc`: unless that is a failure, the n_copies copies of copy_bytes each from copy_from[] are
// enqueued, one behind the other into the pinned output frames; the stream is awaited either way; the first failure is the code and the
// sticky error is cleared — the caller then forgets its frames.  Otherwise the first `count` pinned output frames go to host_outs.
int deliver(const PaddedStream& s, int rc, const uint8_t* const* copy_from, int n_copies, int64_t copy_bytes, const fldr_video_frame* host_outs,
            int count) {
    for (int q = 0; q < n_copies && !rc; ++q)
        rc = (int)hipMemcpyAsync(s.out_host + q * copy_bytes, copy_from[q], (size_t)copy_bytes, hipMemcpyDeviceToHost, s.sm.stream);
    const hipError_t e = hipStreamSynchronize(s.sm.stream);
    if (!rc) rc = (int)e;
    if (rc) { (void)hipGetLastError(); return rc; }
    for (int k = 0; k < count; ++k) unpack_frame(host_outs[k], s.out_host + k * s.frame_bytes, s.format, s.H, s.W, SLOT_PITCH);
    return 0;
}

}  // namespace
