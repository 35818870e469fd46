// libfldr_pack10.so, host side: what a valid fldr_pack10_format is, how long a row of each container is and how its plane must be
// aligned, the two public converters, and what the library puts into the one forward and session text of ../video/yuv_stream_host.h (its
// structs, codes, format check, colour constants and converters), its error strings, and the exported functions as wrappers.  The frame
// checks, packed frames and the stream / device block / pinned block of a session come from ../video/frame_host.h, the colour tables from
// ../video/yuv_color.h (the depth-10 table), so all are those of libfldr_video.so.
#include <hip/hip_runtime.h>

#include "../video/frame_host.h"
#include "pack10_internal.h"

using namespace fldr_pack10_impl;

namespace {

// ---- formats, and the frame rules of frame_host.h for them ---------------------------------------------------------------------------
int check_format(const fldr_pack10_format& f) {
    if ((unsigned)f.container > 2u || (unsigned)f.matrix > 1u || (unsigned)f.range > 1u || f.depth != 10) return FLDR_PACK10_E_FORMAT;
    for (int i = 0; i < 4; ++i) if (f.reserved[i]) return FLDR_PACK10_E_FORMAT;
    return 0;
}

template <> struct FrameRules<fldr_pack10_format> {
    using Frame = fldr_pack10_frame;
    static constexpr int E_PLANE = FLDR_PACK10_E_PLANE, E_PITCH = FLDR_PACK10_E_PITCH;
    static int planes(const fldr_pack10_format&) { return 1; }
    static int64_t row_bytes(const fldr_pack10_format& f, int, int W) {
        if (f.container == FLDR_PACK10_V210) return 16 * (((int64_t)W + 5) / 6);       // whole groups of six pixels
        if (f.container == FLDR_PACK10_Y210) return 8 * (((int64_t)W + 1) / 2);        // Y0 U Y1 V per two pixels
        return 4 * (int64_t)W;                                                         // Y410: one dword per pixel
    }
    static int rows(const fldr_pack10_format&, int, int H) { return H; }
};

// The frame check every function of ../video/yuv_stream_host.h makes (declared before that text so that its calls choose this overload):
// frame_host.h's (a plane, a pitch that covers the row, both even), then the 32-bit containers' unit of 4 bytes.
int check_frame(const fldr_pack10_frame& fr, const fldr_pack10_format& f, int W) {
    CK(check_frame<fldr_pack10_format>(fr, f, W));
    if (f.container != FLDR_PACK10_Y210) {
        if ((uintptr_t)fr.plane[0] & 3) return FLDR_PACK10_E_PLANE;
        if (fr.pitch[0] & 3) return FLDR_PACK10_E_PITCH;
    }
    return 0;
}

}  // namespace

#include "../video/yuv_stream_host.h"

namespace {

const YuvCoeffs& coeffs(const fldr_pack10_format& f) { return fldr_video_impl::YUV_COEFFS_10[f.matrix][f.range]; }

struct Pack10Lib {
    using Format = fldr_pack10_format;
    using Frame = fldr_pack10_frame;
    using Io = fldr_pack10_io;
    using Config = fldr_pack10_session_config;
    static constexpr int E_ARG = FLDR_PACK10_E_ARG, E_FORMAT = FLDR_PACK10_E_FORMAT, E_WORKSPACE = FLDR_PACK10_E_WORKSPACE, E_DEVICE = FLDR_PACK10_E_DEVICE;
    static int check_format(const Format& f) { return ::check_format(f); }
    static int to_planar(const Frame in[2], const Format& f, void* pair, int H, int W, hipStream_t s) {
        return fldr_pack10_impl::to_planar(in, 2, f, coeffs(f), pair, H, W, s);
    }
    static int from_planar(const void* planar, const Frame& out, const Format& f, int H, int W, hipStream_t s) {
        return fldr_pack10_impl::from_planar(planar, out, f, coeffs(f), H, W, s);
    }
};

}  // namespace

struct fldr_pack10_session : Session<Pack10Lib> {};

extern "C" FLDR_PACK10_API int fldr_pack10_version(void) { return FLDR_PACK10_VERSION; }

extern "C" FLDR_PACK10_API const char* fldr_pack10_error_string(int code) {
    switch (code) {
    case 0: return "success";
    case FLDR_PACK10_E_ARG: return "fldr_pack10: bad argument";
    case FLDR_PACK10_E_FORMAT: return "fldr_pack10: unknown container, matrix or range, a depth other than 10, or a non-zero reserved word";
    case FLDR_PACK10_E_PITCH: return "fldr_pack10: pitch shorter than its row, or not a multiple of 4 (v210, Y410) / 2 (Y210)";
    case FLDR_PACK10_E_PLANE: return "fldr_pack10: null plane pointer, or an address that is not a multiple of 4 (v210, Y410) / 2 (Y210)";
    case FLDR_PACK10_E_WORKSPACE: return "fldr_pack10: workspace missing, misaligned or too small";
    case FLDR_PACK10_E_DEVICE: return "fldr_pack10: no such device or out of memory";
    default: return code > -100 && code < 0 ? fldr_model_error_string(code) : code > 0 ? hipGetErrorString((hipError_t)code)
                                                                                      : "fldr_pack10: unknown error";
    }
}

extern "C" FLDR_PACK10_API int fldr_pack10_sizeof(int which) {
    switch (which) {
    case 0: return (int)sizeof(fldr_pack10_format);
    case 1: return (int)sizeof(fldr_pack10_frame);
    case 2: return (int)sizeof(fldr_pack10_io);
    case 3: return (int)sizeof(fldr_pack10_session_config);
    default: return FLDR_PACK10_E_ARG;
    }
}

extern "C" FLDR_PACK10_API int fldr_pack10_to_planar(const fldr_pack10_frame* frames, int n_frames, const fldr_pack10_format* format, void* planar,
                                                     int H, int W, void* stream) {
    if (!frames || !format || !planar || n_frames < 1 || H < 1 || W < 1) return FLDR_PACK10_E_ARG;
    CK(check_format(*format));
    if ((uintptr_t)planar & 1) return FLDR_PACK10_E_ARG;
    for (int f = 0; f < n_frames; ++f) CK(check_frame(frames[f], *format, W));
    const int64_t frame_bytes = 6ll * H * W;
    for (int f = 0; f < n_frames; f += MAX_FRAMES) {
        const int n = n_frames - f < MAX_FRAMES ? n_frames - f : MAX_FRAMES;
        CK(to_planar(frames + f, n, *format, coeffs(*format), (uint8_t*)planar + f * frame_bytes, H, W, (hipStream_t)stream));
    }
    return 0;
}

extern "C" FLDR_PACK10_API int fldr_pack10_from_planar(const void* planar, const fldr_pack10_format* format, const fldr_pack10_frame* out_frame,
                                                       int H, int W, void* stream) {
    if (!planar || !format || !out_frame || H < 1 || W < 1) return FLDR_PACK10_E_ARG;
    CK(check_format(*format));
    if ((uintptr_t)planar & 1) return FLDR_PACK10_E_ARG;
    CK(check_frame(*out_frame, *format, W));
    return from_planar(planar, *out_frame, *format, coeffs(*format), H, W, (hipStream_t)stream);
}

extern "C" FLDR_PACK10_API int64_t fldr_pack10_workspace_bytes(const fldr_model* m, int H, int W, int n_t) { return workspace_bytes<Pack10Lib>(m, H, W, n_t); }

extern "C" FLDR_PACK10_API int fldr_pack10_forward(const fldr_model* m, const fldr_pack10_io* io, void* ws, int64_t ws_bytes, void* stream) {
    return forward<Pack10Lib>(m, io, ws, ws_bytes, stream);
}

extern "C" FLDR_PACK10_API int fldr_pack10_session_create(const fldr_model* m, const fldr_pack10_session_config* cfg, fldr_pack10_session** out) {
    return session_create<Pack10Lib>(m, cfg, out);
}

extern "C" FLDR_PACK10_API int fldr_pack10_session_push(fldr_pack10_session* s, const fldr_pack10_frame* frame, const fldr_pack10_frame* host_outs,
                                                        int* n_out) {
    return session_push<Pack10Lib>(s, frame, host_outs, n_out);
}

extern "C" FLDR_PACK10_API int fldr_pack10_session_reset(fldr_pack10_session* s) { return session_reset<Pack10Lib>(s); }

extern "C" FLDR_PACK10_API void fldr_pack10_session_destroy(fldr_pack10_session* s) { session_destroy(s); }
