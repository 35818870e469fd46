// libfldr_chroma.so, host side: what a valid fldr_chroma_format is and how large its planes are, and what the
// library puts into the one forward and session text of ../video/yuv_stream_host.h (its structs, codes, format check, colour constants and
// converters), its error strings, and the exported functions as wrappers.  The frame checks, packed frames and the stream / device block
// / pinned block of a session come from ../video/frame_host.h, the colour tables from ../video/yuv_color.h, so all are those of
// libfldr_video.so.
#include <hip/hip_runtime.h>

#include "../video/yuv_stream_host.h"
#include "chroma_internal.h"

using namespace fldr_chroma_impl;

namespace {

// ---- formats, and the frame rules of frame_host.h for them ---------------------------------------------------------------------------
bool packed_layout(const fldr_chroma_format& f) { return f.layout == FLDR_CHROMA_UYVY || f.layout == FLDR_CHROMA_YUYV; }

int check_format(const fldr_chroma_format& f) {
    if ((unsigned)f.sampling > 1u || (unsigned)f.layout > 3u || (unsigned)f.matrix > 1u || (unsigned)f.range > 1u) return FLDR_CHROMA_E_FORMAT;
    if (f.depth != 0 && f.depth != 8 && f.depth != 10) return FLDR_CHROMA_E_FORMAT;
    if (packed_layout(f) && (deep(f) || f.sampling != FLDR_CHROMA_422)) return FLDR_CHROMA_E_FORMAT;
    for (int i = 0; i < 3; ++i) if (f.reserved[i]) return FLDR_CHROMA_E_FORMAT;
    return 0;
}

template <> struct FrameRules<fldr_chroma_format> {
    using Frame = fldr_chroma_frame;
    static constexpr int E_PLANE = FLDR_CHROMA_E_PLANE, E_PITCH = FLDR_CHROMA_E_PITCH;
    static int planes(const fldr_chroma_format& f) { return f.layout == FLDR_CHROMA_PLANAR ? 3 : f.layout == FLDR_CHROMA_SEMIPLANAR ? 2 : 1; }
    static int64_t row_bytes(const fldr_chroma_format& f, int p, int W) {
        const int64_t half = (W + 1) / 2, b = deep(f) ? 2 : 1;
        if (packed_layout(f)) return 4 * half;
        const int64_t cw = f.sampling == FLDR_CHROMA_444 ? W : half;
        return b * (p == 0 ? W : (f.layout == FLDR_CHROMA_SEMIPLANAR ? 2 * cw : cw));
    }
    static int rows(const fldr_chroma_format&, int, int H) { return H; }      // no vertical subsampling
    static int unit(const fldr_chroma_format&) { return 0; }
};

const YuvCoeffs& coeffs(const fldr_chroma_format& f) {
    return deep(f) ? fldr_video_impl::YUV_COEFFS_10[f.matrix][f.range] : fldr_video_impl::YUV_COEFFS[f.matrix][f.range];
}

struct ChromaLib : LibDefaults {
    using Format = fldr_chroma_format;
    using Frame = fldr_chroma_frame;
    using Io = fldr_chroma_io;
    using Config = fldr_chroma_session_config;
    static constexpr int E_ARG = FLDR_CHROMA_E_ARG, E_FORMAT = FLDR_CHROMA_E_FORMAT, E_WORKSPACE = FLDR_CHROMA_E_WORKSPACE, E_DEVICE = FLDR_CHROMA_E_DEVICE;
    static constexpr int MAX_FRAMES = fldr_chroma_impl::MAX_FRAMES;
    static int check_format(const Format& f) { return ::check_format(f); }
    static int to_planar(const Frame* in, int n, const Format& f, void* planar, int H, int W, hipStream_t s) {
        return fldr_chroma_impl::to_planar(in, n, f, coeffs(f), planar, H, W, s);
    }
    static int from_planar(const void* planar, const Frame& out, const Format& f, int H, int W, hipStream_t s) {
        return fldr_chroma_impl::from_planar(planar, out, f, coeffs(f), H, W, s);
    }
};

}  // namespace

struct fldr_chroma_session : Session<ChromaLib> {};

extern "C" FLDR_CHROMA_API int fldr_chroma_version(void) { return FLDR_CHROMA_VERSION; }

extern "C" FLDR_CHROMA_API const char* fldr_chroma_error_string(int code) {
    switch (code) {
    case 0: return "success";
    case FLDR_CHROMA_E_ARG: return "fldr_chroma: bad argument";
    case FLDR_CHROMA_E_FORMAT: return "fldr_chroma: unknown sampling, layout, matrix, range or depth, a packed layout that is not 8-bit 4:2:2, or a non-zero reserved word";
    case FLDR_CHROMA_E_PITCH: return "fldr_chroma: plane pitch shorter than its row (or odd at depth 10)";
    case FLDR_CHROMA_E_PLANE: return "fldr_chroma: null plane pointer (or an odd address at depth 10)";
    case FLDR_CHROMA_E_WORKSPACE: return "fldr_chroma: workspace missing, misaligned or too small";
    case FLDR_CHROMA_E_DEVICE: return "fldr_chroma: no such device or out of memory";
    default: return passed_error_string(code, "fldr_chroma: unknown error");
    }
}

extern "C" FLDR_CHROMA_API int fldr_chroma_sizeof(int which) { return struct_sizeof<ChromaLib>(which); }

extern "C" FLDR_CHROMA_API int fldr_chroma_to_planar(const fldr_chroma_frame* frames, int n_frames, const fldr_chroma_format* format, void* planar,
                                                     int H, int W, void* stream) {
    return to_planar_entry<ChromaLib>(frames, n_frames, format, planar, H, W, stream);
}

extern "C" FLDR_CHROMA_API int fldr_chroma_from_planar(const void* planar, const fldr_chroma_format* format, const fldr_chroma_frame* out_frame,
                                                       int H, int W, void* stream) {
    return from_planar_entry<ChromaLib>(planar, format, out_frame, H, W, stream);
}

extern "C" FLDR_CHROMA_API int64_t fldr_chroma_workspace_bytes(const fldr_model* m, int H, int W, int n_t) { return workspace_bytes<ChromaLib>(m, H, W, n_t); }

extern "C" FLDR_CHROMA_API int fldr_chroma_forward(const fldr_model* m, const fldr_chroma_io* io, void* ws, int64_t ws_bytes, void* stream) {
    return forward<ChromaLib>(m, io, ws, ws_bytes, stream);
}

extern "C" FLDR_CHROMA_API int fldr_chroma_session_create(const fldr_model* m, const fldr_chroma_session_config* cfg, fldr_chroma_session** out) {
    return session_create<ChromaLib>(m, cfg, out);
}

extern "C" FLDR_CHROMA_API int fldr_chroma_session_push(fldr_chroma_session* s, const fldr_chroma_frame* frame, const fldr_chroma_frame* host_outs,
                                                        int* n_out) {
    return session_push<ChromaLib>(s, frame, host_outs, n_out);
}

extern "C" FLDR_CHROMA_API int fldr_chroma_session_reset(fldr_chroma_session* s) { return session_reset<ChromaLib>(s); }

extern "C" FLDR_CHROMA_API void fldr_chroma_session_destroy(fldr_chroma_session* s) { session_destroy(s); }
