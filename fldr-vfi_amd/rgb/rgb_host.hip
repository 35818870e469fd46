// libfldr_rgb.so, host side: what a valid fldr_rgb_format is, how long a row of each layout is and how its planes must be aligned, which
// formats may meet under an alpha policy, the two public converters and the alpha pass, and what the library puts into the one forward and session text of
// ../video/yuv_stream_host.h (its structs, codes, format check and converters), its error strings, and the exported functions.  The frame
// checks, packed frames and the stream / device block / pinned block of a session come from ../video/frame_host.h, so they are those of
// libfldr_video.so.  That text's forward does the colour; the alpha of its outputs needs the two input frames and the times, which its
// output converter never sees, so this file's forward runs it and then launches the alpha pass, and the session's push (that text's,
// written again here) calls this forward.
#include <hip/hip_runtime.h>

#include "../video/frame_host.h"
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
};

// The frame check every function of ../video/yuv_stream_host.h makes (declared before that text so that its calls choose this overload):
// frame_host.h's (the planes of the layout, pitches that cover the row, both even at depth 10), then the word layouts' unit of 4 bytes.
int check_frame(const fldr_rgb_frame& fr, const fldr_rgb_format& f, int W) {
    CK(check_frame<fldr_rgb_format>(fr, f, W));
    if (word_layout(f)) {
        if ((uintptr_t)fr.plane[0] & 3) return FLDR_RGB_E_PLANE;
        if (fr.pitch[0] & 3) return FLDR_RGB_E_PITCH;
    }
    return 0;
}

}  // namespace

#include "../video/yuv_stream_host.h"

namespace {

struct RgbLib {
    using Format = fldr_rgb_format;
    using Frame = fldr_rgb_frame;
    using Io = fldr_rgb_io;
    using Config = fldr_rgb_session_config;
    static constexpr int E_ARG = FLDR_RGB_E_ARG, E_FORMAT = FLDR_RGB_E_FORMAT, E_WORKSPACE = FLDR_RGB_E_WORKSPACE, E_DEVICE = FLDR_RGB_E_DEVICE;
    static int check_format(const Format& f) { return ::check_format(f); }
    static int to_planar(const Frame in[2], const Format& f, void* pair, int H, int W, hipStream_t s) {
        return fldr_rgb_impl::to_planar(in, 2, f, pair, H, W, s);
    }
    static int from_planar(const void* planar, const Frame& out, const Format& f, int H, int W, hipStream_t s) {
        return fldr_rgb_impl::from_planar(planar, out, f, H, W, s);
    }
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

// The colour through the shared forward (its outputs carry opaque alpha), then the alpha of the n_t outputs where the policy asks for
// it.  Nothing is enqueued before every argument is checked; a forward the model refuses returns before the alpha pass.
int rgb_forward(const fldr_model* m, const fldr_rgb_io* io, void* ws, int64_t ws_bytes, void* stream) {
    CK(validate_io<RgbLib>(io));
    CK(check_alpha_pair(io->in_format, io->out_format));
    CK(forward<RgbLib>(m, io, ws, ws_bytes, stream));
    return alpha_pass(io->in, io->in_format, io->out, io->n_t, io->out_format, io->t, io->H, io->W, (hipStream_t)stream);
}

}  // namespace

struct fldr_rgb_session : Session<RgbLib> {};

namespace {

// session_push of ../video/yuv_stream_host.h with this library's forward in place of that text's
int rgb_session_push(fldr_rgb_session* s, const fldr_rgb_frame* frame, const fldr_rgb_frame* host_outs, int* n_out) {
    if (!s || !frame || !n_out) return FLDR_RGB_E_ARG;
    *n_out = 0;
    const fldr_rgb_session_config& c = s->cfg;
    const int H = c.H, W = c.W, n_t = c.n_t;
    CK(check_frame(*frame, c.in_format, W));
    if (s->prev >= 0) {
        if (!host_outs) return FLDR_RGB_E_ARG;
        for (int k = 0; k < n_t; ++k) CK(check_frame(host_outs[k], c.out_format, W));
    }
    DeviceGuard g(s->sm.device);
    if (!g.ok) return FLDR_RGB_E_DEVICE;
    const hipStream_t stream = s->sm.stream;
    const int cur = s->prev == 0 ? 1 : 0;                          // the slot not holding the previous frame
    hipError_t e = upload_frame(s->sm, s->slot[cur], s->sm.pinned, s->in_bytes, *frame, c.in_format, H, W);
    int rc = e == hipSuccess ? 0 : (int)e;
    const bool interp = s->prev >= 0;
    uint8_t* out_host = s->sm.pinned + s->in_bytes;
    if (!rc && interp) {
        std::vector<fldr_rgb_frame> outs((size_t)n_t);
        for (int k = 0; k < n_t; ++k) outs[k] = packed(s->out_dev + k * s->out_bytes, c.out_format, H, W);
        fldr_rgb_io io;
        memset(&io, 0, sizeof(io));
        io.H = H; io.W = W;
        io.in_format = c.in_format;
        io.in[0] = packed(s->slot[s->prev], c.in_format, H, W);
        io.in[1] = packed(s->slot[cur], c.in_format, H, W);
        io.out_format = c.out_format;
        io.n_t = n_t; io.t = s->t_dev; io.out = outs.data();
        rc = rgb_forward(s->model, &io, s->ws, s->ws_bytes, stream);
        if (!rc) {
            e = hipMemcpyAsync(out_host, s->out_dev, (size_t)(n_t * s->out_bytes), hipMemcpyDeviceToHost, stream);
            if (e != hipSuccess) rc = (int)e;
        }
    }
    e = hipStreamSynchronize(stream);
    if (!rc && e != hipSuccess) rc = (int)e;
    if (rc) { s->prev = -1; return rc; }                           // the held frame is not to be trusted
    if (interp) {
        for (int k = 0; k < n_t; ++k) unpack_frame(host_outs[k], out_host + k * s->out_bytes, c.out_format, H, W);
        *n_out = n_t;
    }
    s->prev = cur;
    return 0;
}

}  // namespace

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
    default: return code > -100 && code < 0 ? fldr_model_error_string(code) : code > 0 ? hipGetErrorString((hipError_t)code)
                                                                                      : "fldr_rgb: unknown error";
    }
}

extern "C" FLDR_RGB_API int fldr_rgb_sizeof(int which) {
    switch (which) {
    case 0: return (int)sizeof(fldr_rgb_format);
    case 1: return (int)sizeof(fldr_rgb_frame);
    case 2: return (int)sizeof(fldr_rgb_io);
    case 3: return (int)sizeof(fldr_rgb_session_config);
    default: return FLDR_RGB_E_ARG;
    }
}

extern "C" FLDR_RGB_API int fldr_rgb_to_planar(const fldr_rgb_frame* frames, int n_frames, const fldr_rgb_format* format, void* planar, int H, int W,
                                               void* stream) {
    if (!frames || !format || !planar || n_frames < 1 || H < 1 || W < 1) return FLDR_RGB_E_ARG;
    CK(check_format(*format));
    if (words16(*format) && ((uintptr_t)planar & 1)) return FLDR_RGB_E_ARG;
    for (int f = 0; f < n_frames; ++f) CK(check_frame(frames[f], *format, W));
    const int64_t frame_bytes = 3ll * H * W * (words16(*format) ? 2 : 1);
    for (int f = 0; f < n_frames; f += MAX_FRAMES) {
        const int n = n_frames - f < MAX_FRAMES ? n_frames - f : MAX_FRAMES;
        CK(to_planar(frames + f, n, *format, (uint8_t*)planar + f * frame_bytes, H, W, (hipStream_t)stream));
    }
    return 0;
}

extern "C" FLDR_RGB_API int fldr_rgb_from_planar(const void* planar, const fldr_rgb_format* format, const fldr_rgb_frame* out_frame, int H, int W,
                                                 void* stream) {
    if (!planar || !format || !out_frame || H < 1 || W < 1) return FLDR_RGB_E_ARG;
    CK(check_format(*format));
    if (words16(*format) && ((uintptr_t)planar & 1)) return FLDR_RGB_E_ARG;
    CK(check_frame(*out_frame, *format, W));
    return from_planar(planar, *out_frame, *format, H, W, (hipStream_t)stream);
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
    return rgb_forward(m, io, ws, ws_bytes, stream);
}

extern "C" FLDR_RGB_API int fldr_rgb_session_create(const fldr_model* m, const fldr_rgb_session_config* cfg, fldr_rgb_session** out) {
    // the one check that text's create does not make, at the place of its format checks (after its size checks)
    if (cfg && out && cfg->H >= 2 && cfg->W >= 2 && cfg->n_t >= 1 && cfg->device >= 0 && !check_format(cfg->in_format) && !check_format(cfg->out_format)) {
        *out = nullptr;
        CK(check_alpha_pair(cfg->in_format, cfg->out_format));
    }
    return session_create<RgbLib>(m, cfg, out);
}

extern "C" FLDR_RGB_API int fldr_rgb_session_push(fldr_rgb_session* s, const fldr_rgb_frame* frame, const fldr_rgb_frame* host_outs, int* n_out) {
    return rgb_session_push(s, frame, host_outs, n_out);
}

extern "C" FLDR_RGB_API int fldr_rgb_session_reset(fldr_rgb_session* s) { return session_reset<RgbLib>(s); }

extern "C" FLDR_RGB_API void fldr_rgb_session_destroy(fldr_rgb_session* s) { session_destroy(s); }
