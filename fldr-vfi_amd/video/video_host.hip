// libfldr_video.so, host side: the workspace layout, fldr_video_forward (input conversion -> one fldr_model_forward -> n_t output
// conversions) and the session API for streams of host frames.  What a valid format and frame are, and the stream / device block / pinned
// block a session owns, are in frame_host.h (shared with libfldr_rate.so).  The only fldr_* functions called are those of fldr_model.h.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <vector>

#include "frame_host.h"
#include "video_internal.h"

using namespace fldr_video_impl;

namespace {

// host-only checks of a forward's arguments (no model, no device)
int validate_io(const fldr_video_io* io) {
    if (!io) return FLDR_VIDEO_E_ARG;
    if (io->H < 2 || io->W < 2 || io->n_t < 1 || !io->t || !io->out) return FLDR_VIDEO_E_ARG;
    int rc = check_format(io->in_format);
    if (!rc) rc = check_format(io->out_format);
    for (int f = 0; f < 2 && !rc; ++f) rc = check_frame(io->in[f], io->in_format, io->W);
    for (int k = 0; k < io->n_t && !rc; ++k) rc = check_frame(io->out[k], io->out_format, io->W);
    return rc;
}

struct WsLayout { int64_t model, pair, out, out_stride, total; };

// in_bytes / out_bytes: bytes per sample of the planar pair / outputs of THIS forward (the offsets); the total is always that of the
// 16-bit regions, so one size serves every format (fldr_video_workspace_bytes has no format argument)
int64_t plan(const fldr_model* m, int H, int W, int n_t, int in_bytes, int out_bytes, WsLayout& L) {
    if (!m || H < 2 || W < 2 || n_t < 1) return FLDR_VIDEO_E_ARG;
    const int64_t mb = fldr_model_workspace_bytes(m, H, W, n_t);
    if (mb < 0) return mb;
    L.model = 0;
    L.pair = align_up(mb);
    L.out = L.pair + align_up(6ll * H * W * in_bytes);
    L.out_stride = align_up(3ll * H * W * out_bytes);
    L.total = L.pair + align_up(12ll * H * W) + (int64_t)n_t * align_up(6ll * H * W);
    return L.total;
}

const YuvCoeffs& coeffs(const fldr_video_format& f) { return deep(f) ? YUV_COEFFS_10[f.matrix][f.range] : YUV_COEFFS[f.matrix][f.range]; }

}  // namespace

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
    default: return code > -100 && code < 0 ? fldr_model_error_string(code) : code > 0 ? hipGetErrorString((hipError_t)code)
                                                                                      : "fldr_video: unknown error";
    }
}

extern "C" FLDR_VIDEO_API int fldr_video_sizeof(int which) {
    switch (which) {
    case 0: return (int)sizeof(fldr_video_format);
    case 1: return (int)sizeof(fldr_video_frame);
    case 2: return (int)sizeof(fldr_video_io);
    case 3: return (int)sizeof(fldr_video_session_config);
    default: return FLDR_VIDEO_E_ARG;
    }
}

extern "C" FLDR_VIDEO_API int64_t fldr_video_workspace_bytes(const fldr_model* m, int H, int W, int n_t) {
    WsLayout L;
    return plan(m, H, W, n_t, 2, 2, L);
}

extern "C" FLDR_VIDEO_API int fldr_video_forward(const fldr_model* m, const fldr_video_io* io, void* ws, int64_t ws_bytes, void* stream) {
    CK(validate_io(io));
    WsLayout L;
    const bool in10 = deep(io->in_format), out10 = deep(io->out_format);
    const int64_t total = plan(m, io->H, io->W, io->n_t, in10 ? 2 : 1, out10 ? 2 : 1, L);
    if (total < 0) return (int)total;
    if (!ws || ((uintptr_t)ws & (ALIGN - 1)) || ws_bytes < total) return FLDR_VIDEO_E_WORKSPACE;
    const int H = io->H, W = io->W;
    char* w = (char*)ws;
    uint8_t* pair = (uint8_t*)(w + L.pair);
    const hipStream_t s = (hipStream_t)stream;
    std::vector<void*> planar((size_t)io->n_t);
    for (int k = 0; k < io->n_t; ++k) planar[k] = w + L.out + (int64_t)k * L.out_stride;
    // the conversion writes the workspace only: if the model then refuses (a fault flag of an earlier call), no output is touched
    if (in10) CK(yuv420_to_planar_pair10(io->in, io->in_format.layout, coeffs(io->in_format), (uint16_t*)pair, H, W, s));
    else CK(yuv420_to_planar_pair(io->in, io->in_format.layout, coeffs(io->in_format), pair, H, W, s));
    fldr_model_io mio;
    memset(&mio, 0, sizeof(mio));
    mio.batch = 1; mio.H = H; mio.W = W; mio.input = in10 ? FLDR_MODEL_IN_U10_PLANAR : FLDR_MODEL_IN_U8_PLANAR; mio.frames_u8 = pair;
    mio.n_t = io->n_t; mio.t = io->t; mio.output = out10 ? FLDR_MODEL_OUT_U10_PLANAR : FLDR_MODEL_OUT_U8_PLANAR; mio.out = planar.data();
    CK(fldr_model_forward(m, &mio, w + L.model, L.pair, stream));
    for (int k = 0; k < io->n_t; ++k) {
        if (out10) CK(planar_to_yuv420_10((const uint16_t*)planar[k], io->out[k], io->out_format.layout, coeffs(io->out_format), H, W, s));
        else CK(planar_to_yuv420((const uint8_t*)planar[k], io->out[k], io->out_format.layout, coeffs(io->out_format), H, W, s));
    }
    return 0;
}

// ---- sessions -----------------------------------------------------------------------------------------------------------------
struct fldr_video_session {
    const fldr_model* model;
    fldr_video_session_config cfg;
    StreamMem sm;                      // device: slot 0, slot 1, n_t outputs, t, workspace; pinned: one input frame, n_t output frames (packed)
    int64_t in_bytes, out_bytes, ws_bytes;
    uint8_t* slot[2];
    uint8_t* out_dev;
    float* t_dev;
    void* ws;
    int prev;                          // slot holding the previous frame, -1 when none
};

extern "C" FLDR_VIDEO_API int fldr_video_session_create(const fldr_model* m, const fldr_video_session_config* cfg, fldr_video_session** out) {
    if (!cfg || !out) return FLDR_VIDEO_E_ARG;
    *out = nullptr;
    if (cfg->H < 2 || cfg->W < 2 || cfg->n_t < 1 || cfg->device < 0) return FLDR_VIDEO_E_ARG;
    CK(check_format(cfg->in_format));
    CK(check_format(cfg->out_format));
    for (int i = 0; i < 4; ++i) if (cfg->reserved[i]) return FLDR_VIDEO_E_FORMAT;
    if (!m) return FLDR_VIDEO_E_ARG;
    const int H = cfg->H, W = cfg->W, n_t = cfg->n_t;
    const int64_t wsb = fldr_video_workspace_bytes(m, H, W, n_t);
    if (wsb < 0) return (int)wsb;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device >= ndev) { (void)hipGetLastError(); return FLDR_VIDEO_E_DEVICE; }
    fldr_video_session* s = new (std::nothrow) fldr_video_session();
    if (!s) return FLDR_VIDEO_E_DEVICE;
    s->model = m;
    s->cfg = *cfg;
    s->cfg.t = nullptr;
    s->prev = -1;
    s->in_bytes = align_up(packed_bytes(cfg->in_format, H, W));
    s->out_bytes = align_up(packed_bytes(cfg->out_format, H, W));
    s->ws_bytes = wsb;
    DeviceGuard g(cfg->device);
    const int64_t dev_total = 2 * s->in_bytes + n_t * s->out_bytes + align_up(4ll * n_t) + wsb;
    const int64_t host_total = s->in_bytes + n_t * s->out_bytes;
    if (!g.ok || !open_stream_mem(s->sm, cfg->device, dev_total, host_total)) { delete s; return FLDR_VIDEO_E_DEVICE; }
    s->slot[0] = s->sm.dev;
    s->slot[1] = s->slot[0] + s->in_bytes;
    s->out_dev = s->slot[1] + s->in_bytes;
    s->t_dev = (float*)(s->out_dev + n_t * s->out_bytes);
    s->ws = (char*)s->t_dev + align_up(4ll * n_t);
    std::vector<float> t((size_t)n_t);
    for (int k = 0; k < n_t; ++k) t[k] = cfg->t ? cfg->t[k] : (float)(k + 1) / (float)(n_t + 1);
    hipError_t e = hipMemcpyAsync(s->t_dev, t.data(), 4ull * n_t, hipMemcpyHostToDevice, s->sm.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->sm.stream);
    if (e != hipSuccess) { fldr_video_session_destroy(s); return (int)e; }
    *out = s;
    return 0;
}

extern "C" FLDR_VIDEO_API int fldr_video_session_push(fldr_video_session* s, const fldr_video_frame* frame, const fldr_video_frame* host_outs,
                                                      int* n_out) {
    if (!s || !frame || !n_out) return FLDR_VIDEO_E_ARG;
    *n_out = 0;
    const fldr_video_session_config& c = s->cfg;
    const int H = c.H, W = c.W, n_t = c.n_t;
    CK(check_frame(*frame, c.in_format, W));
    if (s->prev >= 0) {
        if (!host_outs) return FLDR_VIDEO_E_ARG;
        for (int k = 0; k < n_t; ++k) CK(check_frame(host_outs[k], c.out_format, W));
    }
    DeviceGuard g(s->sm.device);
    if (!g.ok) return FLDR_VIDEO_E_DEVICE;
    const hipStream_t stream = s->sm.stream;
    const int cur = s->prev == 0 ? 1 : 0;                          // the slot not holding the previous frame
    hipError_t e = upload_frame(s->sm, s->slot[cur], s->sm.pinned, s->in_bytes, *frame, c.in_format, H, W);
    int rc = e == hipSuccess ? 0 : (int)e;
    const bool interp = s->prev >= 0;
    uint8_t* out_host = s->sm.pinned + s->in_bytes;
    if (!rc && interp) {
        std::vector<fldr_video_frame> outs((size_t)n_t);
        for (int k = 0; k < n_t; ++k) outs[k] = packed(s->out_dev + k * s->out_bytes, c.out_format, H, W);
        fldr_video_io io;
        memset(&io, 0, sizeof(io));
        io.H = H; io.W = W;
        io.in_format = c.in_format;
        io.in[0] = packed(s->slot[s->prev], c.in_format, H, W);
        io.in[1] = packed(s->slot[cur], c.in_format, H, W);
        io.out_format = c.out_format;
        io.n_t = n_t; io.t = s->t_dev; io.out = outs.data();
        rc = fldr_video_forward(s->model, &io, s->ws, s->ws_bytes, stream);
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

extern "C" FLDR_VIDEO_API int fldr_video_session_reset(fldr_video_session* s) {
    if (!s) return FLDR_VIDEO_E_ARG;
    s->prev = -1;
    return 0;
}

extern "C" FLDR_VIDEO_API void fldr_video_session_destroy(fldr_video_session* s) {
    if (s) { close_stream_mem(s->sm); delete s; }
}

// ---- converter hooks of the test build (include/fldr_video_test_hooks.h): the two converters alone, behind fldr_video_forward's checks ---
#ifdef FLDR_TEST_HOOKS
#include "fldr_video_test_hooks.h"

extern "C" FLDR_VIDEO_API int fldr_video_debug_to_planar(const fldr_video_frame in[2], const fldr_video_format* format, void* pair, int H, int W,
                                                         void* stream) {
    if (!in || !format || !pair || ((uintptr_t)pair & (ALIGN - 1)) || H < 2 || W < 2) return FLDR_VIDEO_E_ARG;
    CK(check_format(*format));
    for (int f = 0; f < 2; ++f) CK(check_frame(in[f], *format, W));
    const hipStream_t s = (hipStream_t)stream;
    if (deep(*format)) return yuv420_to_planar_pair10(in, format->layout, coeffs(*format), (uint16_t*)pair, H, W, s);
    return yuv420_to_planar_pair(in, format->layout, coeffs(*format), (uint8_t*)pair, H, W, s);
}

extern "C" FLDR_VIDEO_API int fldr_video_debug_from_planar(const void* planar, const fldr_video_frame* out_frame, const fldr_video_format* format,
                                                           int H, int W, void* stream) {
    if (!planar || !out_frame || !format || ((uintptr_t)planar & (ALIGN - 1)) || H < 2 || W < 2) return FLDR_VIDEO_E_ARG;
    CK(check_format(*format));
    CK(check_frame(*out_frame, *format, W));
    const hipStream_t s = (hipStream_t)stream;
    if (deep(*format)) return planar_to_yuv420_10((const uint16_t*)planar, *out_frame, format->layout, coeffs(*format), H, W, s);
    return planar_to_yuv420((const uint8_t*)planar, *out_frame, format->layout, coeffs(*format), H, W, s);
}

extern "C" FLDR_VIDEO_API int fldr_video_debug_last_path(void) { return g_last_path; }
#endif
