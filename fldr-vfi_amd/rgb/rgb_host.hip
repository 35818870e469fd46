// libfldr_rgb.so, host side: what a valid fldr_rgb_format is, how long a row of each layout is and how its planes must be aligned, which
// formats may meet under an alpha policy, the alpha pass, and what the library puts into the one forward, session and converter text of
// ../video/yuv_stream_host.h (its structs, codes, format check, converters, its rule for the format pair and its pass after the outputs),
// its error strings, and the exported functions as wrappers.  The frame checks, packed frames and the stream / device block / pinned
// block of a session come from ../video/frame_host.h, so they are those of libfldr_video.so.  That text's forward does the colour; the
// alpha of its outputs needs the two input frames and the times, which its output converter never sees, so the alpha pass runs as the
// forward's pass after the outputs.
#include <hip/hip_runtime.h>

#include "../video/yuv_stream_host.h"
#include "rgb_internal.h"

using namespace fldr_rgb_impl;

namespace {

// ---- formats, and the frame rules of frame_host.h for them ---------------------------------------------------------------------------
int check_format(const fldr_rgb_format& f) {
    if ((unsigned)f.layout > (unsigned)FLDR_RGB_GBRAP || (unsigned)f.alpha > (unsigned)FLDR_RGB_ALPHA_BLEND) return FLDR_RGB_E_FORMAT;
    if (f.layout <= FLDR_RGB_ABGR ? (f.depth != 0 && f.depth != 8)
        : f.layout <= FLDR_RGB_X2BGR10 ? f.depth != 10 : (f.depth != 8 && f.depth != 10)) return FLDR_RGB_E_FORMAT;
    for (int i = 0; i < 5; ++i) if (f.reserved[i]) return FLDR_RGB_E_FORMAT;
    return 0;
}

// does a forward into `out` launch the alpha pass (out.alpha asks for the inputs' alpha and out has somewhere to put it)?
bool wants_alpha(const fldr_rgb_format& out) { return out.alpha != FLDR_RGB_ALPHA_OPAQUE && alpha_bits(out) != 0; }

// NEARER / BLEND need an input with alpha of the output's width (both formats valid)
int check_alpha_pair(const fldr_rgb_format& in, const fldr_rgb_format& out) {
    return wants_alpha(out) && alpha_bits(in) != alpha_bits(out) ? FLDR_RGB_E_FORMAT : 0;
}

template <> struct FrameRules<fldr_rgb_format> {
    using Frame = fldr_rgb_frame;
    static constexpr int E_PLANE = FLDR_RGB_E_PLANE, E_PITCH = FLDR_RGB_E_PITCH;
    static int planes(const fldr_rgb_format& f) { return word_layout(f) ? 1 : f.layout == FLDR_RGB_GBRP ? 3 : 4; }
    static int64_t row_bytes(const fldr_rgb_format& f, int, int W) { return word_layout(f) ? 4 * (int64_t)W : (int64_t)W * (words16(f) ? 2 : 1); }
    static int rows(const fldr_rgb_format&, int, int H) { return H; }
    static int unit(const fldr_rgb_format& f) { return word_layout(f) ? 4 : 0; }
};

// The alpha of n frames `out` (arguments checked by the caller): one launch per ALPHA_MAX_OUT outputs; nothing where the policy is
// OPAQUE or the out layout has no alpha.
int alpha_pass(const fldr_rgb_frame in[2], const fldr_rgb_format& fin, const fldr_rgb_frame* out, int n, const fldr_rgb_format& fout,
               const float* t, int H, int W, hipStream_t stream) {
    if (!wants_alpha(fout)) return 0;
    for (int k = 0; k < n; k += ALPHA_MAX_OUT)
        CK(write_alpha(in, fin, out + k, n - k < ALPHA_MAX_OUT ? n - k : ALPHA_MAX_OUT, fout, t + k, H, W, stream));
    return 0;
}

struct RgbLib : LibDefaults {
    using Format = fldr_rgb_format;
    using Frame = fldr_rgb_frame;
    using Io = fldr_rgb_io;
    using Config = fldr_rgb_session_config;
    static constexpr int E_ARG = FLDR_RGB_E_ARG, E_FORMAT = FLDR_RGB_E_FORMAT, E_WORKSPACE = FLDR_RGB_E_WORKSPACE, E_DEVICE = FLDR_RGB_E_DEVICE;
    static constexpr int MAX_FRAMES = fldr_rgb_impl::MAX_FRAMES;
    static int check_format(const Format& f) { return ::check_format(f); }
    static int to_planar(const Frame* in, int n, const Format& f, void* planar, int H, int W, hipStream_t s) {
        return fldr_rgb_impl::to_planar(in, n, f, planar, H, W, s);
    }
    static int from_planar(const void* planar, const Frame& out, const Format& f, int H, int W, hipStream_t s) {
        return fldr_rgb_impl::from_planar(planar, out, f, H, W, s);
    }
    static int check_pair(const Format& in, const Format& out) { return check_alpha_pair(in, out); }
    // the forward's outputs carry opaque alpha: the alpha of the n_t outputs where the policy asks for it
    static int after_outputs(const Io& io, hipStream_t s) {
        return alpha_pass(io.in, io.in_format, io.out, io.n_t, io.out_format, io.t, io.H, io.W, s);
    }
};

}  // namespace

struct fldr_rgb_session : Session<RgbLib> {};

extern "C" FLDR_RGB_API int fldr_rgb_version(void) { return FLDR_RGB_VERSION; }

extern "C" FLDR_RGB_API const char* fldr_rgb_error_string(int code) {
    switch (code) {
    case 0: return "success";
    case FLDR_RGB_E_ARG: return "fldr_rgb: bad argument";
    case FLDR_RGB_E_FORMAT: return "fldr_rgb: unknown layout / depth pair or alpha policy, a non-zero reserved word, or alpha asked of an input without alpha of the output's width";
    case FLDR_RGB_E_PITCH: return "fldr_rgb: pitch shorter than its row, or not a multiple of 4 (word layouts) / 2 (planar, depth 10)";
    case FLDR_RGB_E_PLANE: return "fldr_rgb: null plane pointer, or an address that is not a multiple of 4 (word layouts) / 2 (planar, depth 10)";
    case FLDR_RGB_E_WORKSPACE: return "fldr_rgb: workspace missing, misaligned or too small";
    case FLDR_RGB_E_DEVICE: return "fldr_rgb: no such device or out of memory";
    default: return passed_error_string(code, "fldr_rgb: unknown error");
    }
}

extern "C" FLDR_RGB_API int fldr_rgb_sizeof(int which) { return struct_sizeof<RgbLib>(which); }

extern "C" FLDR_RGB_API int fldr_rgb_to_planar(const fldr_rgb_frame* frames, int n_frames, const fldr_rgb_format* format, void* planar, int H, int W,
                                               void* stream) {
    return to_planar_entry<RgbLib>(frames, n_frames, format, planar, H, W, stream);
}

extern "C" FLDR_RGB_API int fldr_rgb_from_planar(const void* planar, const fldr_rgb_format* format, const fldr_rgb_frame* out_frame, int H, int W,
                                                 void* stream) {
    return from_planar_entry<RgbLib>(planar, format, out_frame, H, W, stream);
}

extern "C" FLDR_RGB_API int fldr_rgb_alpha(const fldr_rgb_frame* in, const fldr_rgb_format* in_format, const fldr_rgb_frame* out, int n_out,
                                           const fldr_rgb_format* out_format, const float* t, int H, int W, void* stream) {
    if (!in || !in_format || !out || !out_format || !t || n_out < 1 || H < 1 || W < 1) return FLDR_RGB_E_ARG;
    CK(check_format(*in_format));
    CK(check_format(*out_format));
    CK(check_alpha_pair(*in_format, *out_format));
    for (int f = 0; f < 2; ++f) CK(check_frame(in[f], *in_format, W));
    for (int k = 0; k < n_out; ++k) CK(check_frame(out[k], *out_format, W));
    return alpha_pass(in, *in_format, out, n_out, *out_format, t, H, W, (hipStream_t)stream);
}

extern "C" FLDR_RGB_API int64_t fldr_rgb_workspace_bytes(const fldr_model* m, int H, int W, int n_t) { return workspace_bytes<RgbLib>(m, H, W, n_t); }

extern "C" FLDR_RGB_API int fldr_rgb_forward(const fldr_model* m, const fldr_rgb_io* io, void* ws, int64_t ws_bytes, void* stream) {
    return forward<RgbLib>(m, io, ws, ws_bytes, stream);
}

extern "C" FLDR_RGB_API int fldr_rgb_session_create(const fldr_model* m, const fldr_rgb_session_config* cfg, fldr_rgb_session** out) {
    return session_create<RgbLib>(m, cfg, out);
}

extern "C" FLDR_RGB_API int fldr_rgb_session_push(fldr_rgb_session* s, const fldr_rgb_frame* frame, const fldr_rgb_frame* host_outs, int* n_out) {
    return session_push<RgbLib>(s, frame, host_outs, n_out);
}

extern "C" FLDR_RGB_API int fldr_rgb_session_reset(fldr_rgb_session* s) { return session_reset<RgbLib>(s); }

extern "C" FLDR_RGB_API void fldr_rgb_session_destroy(fldr_rgb_session* s) { session_destroy(s); }
