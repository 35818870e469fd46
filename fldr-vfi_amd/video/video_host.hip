// libfldr_video.so, host side: what the library puts into the one forward and session text of yuv_stream_host.h (its structs, codes,
// format check, colour constants and the two converters), its error strings, and the exported functions as wrappers.  What a valid format
// and frame are, and the stream / device block / pinned block a session owns, are in frame_host.h (shared with libfldr_rate.so).
#include <hip/hip_runtime.h>

#include "video_internal.h"
#include "yuv_stream_host.h"

using namespace fldr_video_impl;

namespace {

const YuvCoeffs& coeffs(const fldr_video_format& f) { return deep(f) ? YUV_COEFFS_10[f.matrix][f.range] : YUV_COEFFS[f.matrix][f.range]; }

struct VideoLib : LibDefaults {
    using Format = fldr_video_format;
    using Frame = fldr_video_frame;
    using Io = fldr_video_io;
    using Config = fldr_video_session_config;
    static constexpr int E_ARG = FLDR_VIDEO_E_ARG, E_FORMAT = FLDR_VIDEO_E_FORMAT, E_WORKSPACE = FLDR_VIDEO_E_WORKSPACE, E_DEVICE = FLDR_VIDEO_E_DEVICE;
    static int check_format(const Format& f) { return ::check_format(f); }
    static int to_planar(const Frame* in, int, const Format& f, void* pair, int H, int W, hipStream_t s) {      // always the pair
        return yuv420_to_planar_pair(in, f, coeffs(f), pair, H, W, s);
    }
    static int from_planar(const void* planar, const Frame& out, const Format& f, int H, int W, hipStream_t s) {
        return planar_to_yuv420(planar, out, f, coeffs(f), H, W, s);
    }
};

}  // namespace

struct fldr_video_session : Session<VideoLib> {};

extern "C" FLDR_VIDEO_API int fldr_video_version(void) { return FLDR_VIDEO_VERSION; }

extern "C" FLDR_VIDEO_API const char* fldr_video_error_string(int code) {
    switch (code) {
    case 0: return "success";
    case FLDR_VIDEO_E_ARG: return "fldr_video: bad argument";
    case FLDR_VIDEO_E_FORMAT: return "fldr_video: unknown layout, matrix, range or depth, or a non-zero reserved word";
    case FLDR_VIDEO_E_PITCH: return "fldr_video: plane pitch shorter than its row (or odd at depth 10)";
    case FLDR_VIDEO_E_PLANE: return "fldr_video: null plane pointer (or an odd address at depth 10)";
    case FLDR_VIDEO_E_WORKSPACE: return "fldr_video: workspace missing, misaligned or too small";
    case FLDR_VIDEO_E_DEVICE: return "fldr_video: no such device or out of memory";
    default: return passed_error_string(code, "fldr_video: unknown error");
    }
}

extern "C" FLDR_VIDEO_API int fldr_video_sizeof(int which) { return struct_sizeof<VideoLib>(which); }

extern "C" FLDR_VIDEO_API int64_t fldr_video_workspace_bytes(const fldr_model* m, int H, int W, int n_t) { return workspace_bytes<VideoLib>(m, H, W, n_t); }

extern "C" FLDR_VIDEO_API int fldr_video_forward(const fldr_model* m, const fldr_video_io* io, void* ws, int64_t ws_bytes, void* stream) {
    return forward<VideoLib>(m, io, ws, ws_bytes, stream);
}

extern "C" FLDR_VIDEO_API int fldr_video_session_create(const fldr_model* m, const fldr_video_session_config* cfg, fldr_video_session** out) {
    return session_create<VideoLib>(m, cfg, out);
}

extern "C" FLDR_VIDEO_API int fldr_video_session_push(fldr_video_session* s, const fldr_video_frame* frame, const fldr_video_frame* host_outs,
                                                      int* n_out) {
    return session_push<VideoLib>(s, frame, host_outs, n_out);
}

extern "C" FLDR_VIDEO_API int fldr_video_session_reset(fldr_video_session* s) { return session_reset<VideoLib>(s); }

extern "C" FLDR_VIDEO_API void fldr_video_session_destroy(fldr_video_session* s) { session_destroy(s); }

// ---- converter hooks of the test build (include/fldr_video_test_hooks.h): the two converters alone, behind fldr_video_forward's checks ---
#ifdef FLDR_TEST_HOOKS
#include "fldr_video_test_hooks.h"

extern "C" FLDR_VIDEO_API int fldr_video_debug_to_planar(const fldr_video_frame in[2], const fldr_video_format* format, void* pair, int H, int W,
                                                         void* stream) {
    if (!in || !format || !pair || ((uintptr_t)pair & (ALIGN - 1)) || H < 2 || W < 2) return FLDR_VIDEO_E_ARG;
    CK(check_format(*format));
    for (int f = 0; f < 2; ++f) CK(check_frame(in[f], *format, W));
    return VideoLib::to_planar(in, 2, *format, pair, H, W, (hipStream_t)stream);
}

extern "C" FLDR_VIDEO_API int fldr_video_debug_from_planar(const void* planar, const fldr_video_frame* out_frame, const fldr_video_format* format,
                                                           int H, int W, void* stream) {
    if (!planar || !out_frame || !format || ((uintptr_t)planar & (ALIGN - 1)) || H < 2 || W < 2) return FLDR_VIDEO_E_ARG;
    CK(check_format(*format));
    CK(check_frame(*out_frame, *format, W));
    return VideoLib::from_planar(planar, *out_frame, *format, H, W, (hipStream_t)stream);
}

extern "C" FLDR_VIDEO_API int fldr_video_debug_last_path(void) { return g_last_path; }
#endif
