// libfldr_pack10.so, host side: what a valid fldr_pack10_format is, how long a row of each container is and how its plane must be
// aligned, and what the library puts into the one forward, session and converter text of ../video/yuv_stream_host.h (its structs,
// codes, format check, colour constants and converters), its error strings, and the exported functions as wrappers.  The frame
// checks, packed frames and the stream / device block / pinned block of a session come from ../video/frame_host.h, the colour tables from
// ../video/yuv_color.h (the depth-10 table), so all are those of libfldr_video.so.
#include <hip/hip_runtime.h>

#include "../video/yuv_stream_host.h"
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
    static int unit(const fldr_pack10_format& f) { return f.container == FLDR_PACK10_Y210 ? 0 : 4; }       // v210, Y410: 32-bit words
};

const YuvCoeffs& coeffs(const fldr_pack10_format& f) { return fldr_video_impl::YUV_COEFFS_10[f.matrix][f.range]; }

struct Pack10Lib : LibDefaults {
    using Format = fldr_pack10_format;
    using Frame = fldr_pack10_frame;
    using Io = fldr_pack10_io;
    using Config = fldr_pack10_session_config;
    static constexpr int E_ARG = FLDR_PACK10_E_ARG, E_FORMAT = FLDR_PACK10_E_FORMAT, E_WORKSPACE = FLDR_PACK10_E_WORKSPACE, E_DEVICE = FLDR_PACK10_E_DEVICE;
    static constexpr int MAX_FRAMES = fldr_pack10_impl::MAX_FRAMES;
    static int check_format(const Format& f) { return ::check_format(f); }
    static int to_planar(const Frame* in, int n, const Format& f, void* planar, int H, int W, hipStream_t s) {
        return fldr_pack10_impl::to_planar(in, n, f, coeffs(f), planar, H, W, s);
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
    default: return passed_error_string(code, "fldr_pack10: unknown error");
    }
}

extern "C" FLDR_PACK10_API int fldr_pack10_sizeof(int which) { return struct_sizeof<Pack10Lib>(which); }

extern "C" FLDR_PACK10_API int fldr_pack10_to_planar(const fldr_pack10_frame* frames, int n_frames, const fldr_pack10_format* format, void* planar,
                                                     int H, int W, void* stream) {
    return to_planar_entry<Pack10Lib>(frames, n_frames, format, planar, H, W, stream);
}

extern "C" FLDR_PACK10_API int fldr_pack10_from_planar(const void* planar, const fldr_pack10_format* format, const fldr_pack10_frame* out_frame,
                                                       int H, int W, void* stream) {
    return from_planar_entry<Pack10Lib>(planar, format, out_frame, H, W, stream);
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
