// libfldr_chroma.so, host side: what a valid fldr_chroma_format and frame are, the two public converters, the workspace layout,
// fldr_chroma_forward (input conversion -> one fldr_model_forward -> n_t output conversions) and the session API for streams of host
// frames.  The stream / device block / pinned block a session owns and the alignment rule come from ../video/frame_host.h, the colour
// tables from ../video/yuv_color.h, so both are those of libfldr_video.so.  The only fldr_* functions called are those of fldr_model.h.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <vector>

#include "../video/frame_host.h"
#include "chroma_internal.h"

using namespace fldr_chroma_impl;

namespace {

// ---- formats and frames (the rules of frame_host.h, for fldr_chroma_format) ----------------------------------------------------------
bool deep(const fldr_chroma_format& f) { return f.depth == 10; }          // 16-bit words (depth 0 is an alias of 8)
bool packed_layout(const fldr_chroma_format& f) { return f.layout == FLDR_CHROMA_UYVY || f.layout == FLDR_CHROMA_YUYV; }
int planes_of(const fldr_chroma_format& f) { return f.layout == FLDR_CHROMA_PLANAR ? 3 : f.layout == FLDR_CHROMA_SEMIPLANAR ? 2 : 1; }

int check_format(const fldr_chroma_format& f) {
    if ((unsigned)f.sampling > 1u || (unsigned)f.layout > 3u || (unsigned)f.matrix > 1u || (unsigned)f.range > 1u) return FLDR_CHROMA_E_FORMAT;
    if (f.depth != 0 && f.depth != 8 && f.depth != 10) return FLDR_CHROMA_E_FORMAT;
    if (packed_layout(f) && (deep(f) || f.sampling != FLDR_CHROMA_422)) return FLDR_CHROMA_E_FORMAT;
    for (int i = 0; i < 3; ++i) if (f.reserved[i]) return FLDR_CHROMA_E_FORMAT;
    return 0;
}

// bytes per row of plane p of a frame of width W
int64_t row_bytes(const fldr_chroma_format& f, int p, int W) {
    const int64_t half = (W + 1) / 2, b = deep(f) ? 2 : 1;
    if (packed_layout(f)) return 4 * half;
    const int64_t cw = f.sampling == FLDR_CHROMA_444 ? W : half;
    return b * (p == 0 ? W : (f.layout == FLDR_CHROMA_SEMIPLANAR ? 2 * cw : cw));
}

int check_frame(const fldr_chroma_frame& fr, const fldr_chroma_format& f, int W) {
    for (int p = 0; p < planes_of(f); ++p) if (!fr.plane[p] || (deep(f) && ((uintptr_t)fr.plane[p] & 1))) return FLDR_CHROMA_E_PLANE;
    for (int p = 0; p < planes_of(f); ++p)
        if (fr.pitch[p] < row_bytes(f, p, W) || (deep(f) && (fr.pitch[p] & 1))) return FLDR_CHROMA_E_PITCH;
    return 0;
}

// packed planes of one frame (pitch = row bytes, every plane H rows) starting at `base`
fldr_chroma_frame packed(uint8_t* base, const fldr_chroma_format& fmt, int H, int W) {
    fldr_chroma_frame f;
    memset(&f, 0, sizeof(f));
    int64_t off = 0;
    for (int p = 0; p < planes_of(fmt); ++p) {
        f.plane[p] = base + off;
        f.pitch[p] = row_bytes(fmt, p, W);
        off += f.pitch[p] * H;
    }
    return f;
}

int64_t packed_bytes(const fldr_chroma_format& fmt, int H, int W) {
    int64_t n = 0;
    for (int p = 0; p < planes_of(fmt); ++p) n += row_bytes(fmt, p, W) * H;
    return n;
}

// rows of every plane from `src` (any pitches) to `dst` (any pitches), on the host
void copy_planes(const fldr_chroma_frame& dst, const fldr_chroma_frame& src, const fldr_chroma_format& fmt, int H, int W) {
    for (int p = 0; p < planes_of(fmt); ++p) {
        const int64_t rb = row_bytes(fmt, p, W);
        for (int64_t r = 0; r < H; ++r)
            memcpy((uint8_t*)dst.plane[p] + r * dst.pitch[p], (const uint8_t*)src.plane[p] + r * src.pitch[p], (size_t)rb);
    }
}

const YuvCoeffs& coeffs(const fldr_chroma_format& f) {
    return deep(f) ? fldr_video_impl::YUV_COEFFS_10[f.matrix][f.range] : fldr_video_impl::YUV_COEFFS[f.matrix][f.range];
}

// host-only checks of a forward's arguments (no model, no device)
int validate_io(const fldr_chroma_io* io) {
    if (!io) return FLDR_CHROMA_E_ARG;
    if (io->H < 2 || io->W < 2 || io->n_t < 1 || !io->t || !io->out) return FLDR_CHROMA_E_ARG;
    int rc = check_format(io->in_format);
    if (!rc) rc = check_format(io->out_format);
    for (int f = 0; f < 2 && !rc; ++f) rc = check_frame(io->in[f], io->in_format, io->W);
    for (int k = 0; k < io->n_t && !rc; ++k) rc = check_frame(io->out[k], io->out_format, io->W);
    return rc;
}

struct WsLayout { int64_t model, pair, out, out_stride, total; };

// in_bytes / out_bytes: bytes per sample of the planar pair / outputs of THIS forward (the offsets); the total is always that of the
// 16-bit regions, so one size serves every format
int64_t plan(const fldr_model* m, int H, int W, int n_t, int in_bytes, int out_bytes, WsLayout& L) {
    if (!m || H < 2 || W < 2 || n_t < 1) return FLDR_CHROMA_E_ARG;
    const int64_t mb = fldr_model_workspace_bytes(m, H, W, n_t);
    if (mb < 0) return mb;
    L.model = 0;
    L.pair = align_up(mb);
    L.out = L.pair + align_up(6ll * H * W * in_bytes);
    L.out_stride = align_up(3ll * H * W * out_bytes);
    L.total = L.pair + align_up(12ll * H * W) + (int64_t)n_t * align_up(6ll * H * W);
    return L.total;
}

}  // namespace

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
    default: return code > -100 && code < 0 ? fldr_model_error_string(code) : code > 0 ? hipGetErrorString((hipError_t)code)
                                                                                      : "fldr_chroma: unknown error";
    }
}

extern "C" FLDR_CHROMA_API int fldr_chroma_sizeof(int which) {
    switch (which) {
    case 0: return (int)sizeof(fldr_chroma_format);
    case 1: return (int)sizeof(fldr_chroma_frame);
    case 2: return (int)sizeof(fldr_chroma_io);
    case 3: return (int)sizeof(fldr_chroma_session_config);
    default: return FLDR_CHROMA_E_ARG;
    }
}

extern "C" FLDR_CHROMA_API int fldr_chroma_to_planar(const fldr_chroma_frame* frames, int n_frames, const fldr_chroma_format* format, void* planar,
                                                     int H, int W, void* stream) {
    if (!frames || !format || !planar || n_frames < 1 || H < 1 || W < 1) return FLDR_CHROMA_E_ARG;
    CK(check_format(*format));
    if (deep(*format) && ((uintptr_t)planar & 1)) return FLDR_CHROMA_E_ARG;
    for (int f = 0; f < n_frames; ++f) CK(check_frame(frames[f], *format, W));
    const int64_t frame_bytes = 3ll * H * W * (deep(*format) ? 2 : 1);
    for (int f = 0; f < n_frames; f += MAX_FRAMES) {
        const int n = n_frames - f < MAX_FRAMES ? n_frames - f : MAX_FRAMES;
        CK(to_planar(frames + f, n, *format, coeffs(*format), (uint8_t*)planar + f * frame_bytes, H, W, (hipStream_t)stream));
    }
    return 0;
}

extern "C" FLDR_CHROMA_API int fldr_chroma_from_planar(const void* planar, const fldr_chroma_format* format, const fldr_chroma_frame* out_frame,
                                                       int H, int W, void* stream) {
    if (!planar || !format || !out_frame || H < 1 || W < 1) return FLDR_CHROMA_E_ARG;
    CK(check_format(*format));
    if (deep(*format) && ((uintptr_t)planar & 1)) return FLDR_CHROMA_E_ARG;
    CK(check_frame(*out_frame, *format, W));
    return from_planar(planar, *out_frame, *format, coeffs(*format), H, W, (hipStream_t)stream);
}

extern "C" FLDR_CHROMA_API int64_t fldr_chroma_workspace_bytes(const fldr_model* m, int H, int W, int n_t) {
    WsLayout L;
    return plan(m, H, W, n_t, 2, 2, L);
}

extern "C" FLDR_CHROMA_API int fldr_chroma_forward(const fldr_model* m, const fldr_chroma_io* io, void* ws, int64_t ws_bytes, void* stream) {
    CK(validate_io(io));
    WsLayout L;
    const bool in10 = deep(io->in_format), out10 = deep(io->out_format);
    const int64_t total = plan(m, io->H, io->W, io->n_t, in10 ? 2 : 1, out10 ? 2 : 1, L);
    if (total < 0) return (int)total;
    if (!ws || ((uintptr_t)ws & (ALIGN - 1)) || ws_bytes < total) return FLDR_CHROMA_E_WORKSPACE;
    const int H = io->H, W = io->W;
    char* w = (char*)ws;
    void* pair = w + L.pair;
    const hipStream_t s = (hipStream_t)stream;
    std::vector<void*> planar((size_t)io->n_t);
    for (int k = 0; k < io->n_t; ++k) planar[k] = w + L.out + (int64_t)k * L.out_stride;
    // the conversion writes the workspace only: if the model then refuses (a fault flag of an earlier call), no output is touched
    CK(to_planar(io->in, 2, io->in_format, coeffs(io->in_format), pair, H, W, s));
    fldr_model_io mio;
    memset(&mio, 0, sizeof(mio));
    mio.batch = 1; mio.H = H; mio.W = W; mio.input = in10 ? FLDR_MODEL_IN_U10_PLANAR : FLDR_MODEL_IN_U8_PLANAR; mio.frames_u8 = (const uint8_t*)pair;
    mio.n_t = io->n_t; mio.t = io->t; mio.output = out10 ? FLDR_MODEL_OUT_U10_PLANAR : FLDR_MODEL_OUT_U8_PLANAR; mio.out = planar.data();
    CK(fldr_model_forward(m, &mio, w + L.model, L.pair, stream));
    for (int k = 0; k < io->n_t; ++k) CK(from_planar(planar[k], io->out[k], io->out_format, coeffs(io->out_format), H, W, s));
    return 0;
}

// ---- sessions -----------------------------------------------------------------------------------------------------------------
struct fldr_chroma_session {
    const fldr_model* model;
    fldr_chroma_session_config cfg;
    StreamMem sm;                      // device: slot 0, slot 1, n_t outputs, t, workspace; pinned: one input frame, n_t output frames (packed)
    int64_t in_bytes, out_bytes, ws_bytes;
    uint8_t* slot[2];
    uint8_t* out_dev;
    float* t_dev;
    void* ws;
    int prev;                          // slot holding the previous frame, -1 when none
};

extern "C" FLDR_CHROMA_API int fldr_chroma_session_create(const fldr_model* m, const fldr_chroma_session_config* cfg, fldr_chroma_session** out) {
    if (!cfg || !out) return FLDR_CHROMA_E_ARG;
    *out = nullptr;
    if (cfg->H < 2 || cfg->W < 2 || cfg->n_t < 1 || cfg->device < 0) return FLDR_CHROMA_E_ARG;
    CK(check_format(cfg->in_format));
    CK(check_format(cfg->out_format));
    for (int i = 0; i < 4; ++i) if (cfg->reserved[i]) return FLDR_CHROMA_E_FORMAT;
    if (!m) return FLDR_CHROMA_E_ARG;
    const int H = cfg->H, W = cfg->W, n_t = cfg->n_t;
    const int64_t wsb = fldr_chroma_workspace_bytes(m, H, W, n_t);
    if (wsb < 0) return (int)wsb;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device >= ndev) { (void)hipGetLastError(); return FLDR_CHROMA_E_DEVICE; }
    fldr_chroma_session* s = new (std::nothrow) fldr_chroma_session();
    if (!s) return FLDR_CHROMA_E_DEVICE;
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
    if (!g.ok || !open_stream_mem(s->sm, cfg->device, dev_total, host_total)) { delete s; return FLDR_CHROMA_E_DEVICE; }
    s->slot[0] = s->sm.dev;
    s->slot[1] = s->slot[0] + s->in_bytes;
    s->out_dev = s->slot[1] + s->in_bytes;
    s->t_dev = (float*)(s->out_dev + n_t * s->out_bytes);
    s->ws = (char*)s->t_dev + align_up(4ll * n_t);
    std::vector<float> t((size_t)n_t);
    for (int k = 0; k < n_t; ++k) t[k] = cfg->t ? cfg->t[k] : (float)(k + 1) / (float)(n_t + 1);
    hipError_t e = hipMemcpyAsync(s->t_dev, t.data(), 4ull * n_t, hipMemcpyHostToDevice, s->sm.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->sm.stream);
    if (e != hipSuccess) { fldr_chroma_session_destroy(s); return (int)e; }
    *out = s;
    return 0;
}

extern "C" FLDR_CHROMA_API int fldr_chroma_session_push(fldr_chroma_session* s, const fldr_chroma_frame* frame, const fldr_chroma_frame* host_outs,
                                                        int* n_out) {
    if (!s || !frame || !n_out) return FLDR_CHROMA_E_ARG;
    *n_out = 0;
    const fldr_chroma_session_config& c = s->cfg;
    const int H = c.H, W = c.W, n_t = c.n_t;
    CK(check_frame(*frame, c.in_format, W));
    if (s->prev >= 0) {
        if (!host_outs) return FLDR_CHROMA_E_ARG;
        for (int k = 0; k < n_t; ++k) CK(check_frame(host_outs[k], c.out_format, W));
    }
    DeviceGuard g(s->sm.device);
    if (!g.ok) return FLDR_CHROMA_E_DEVICE;
    const hipStream_t stream = s->sm.stream;
    const int cur = s->prev == 0 ? 1 : 0;                          // the slot not holding the previous frame
    // one host frame (any pitches) -> packed in the pinned block -> enqueued to its slot
    copy_planes(packed(s->sm.pinned, c.in_format, H, W), *frame, c.in_format, H, W);
    hipError_t e = hipMemcpyAsync(s->slot[cur], s->sm.pinned, (size_t)s->in_bytes, hipMemcpyHostToDevice, stream);
    int rc = e == hipSuccess ? 0 : (int)e;
    const bool interp = s->prev >= 0;
    uint8_t* out_host = s->sm.pinned + s->in_bytes;
    if (!rc && interp) {
        std::vector<fldr_chroma_frame> outs((size_t)n_t);
        for (int k = 0; k < n_t; ++k) outs[k] = packed(s->out_dev + k * s->out_bytes, c.out_format, H, W);
        fldr_chroma_io io;
        memset(&io, 0, sizeof(io));
        io.H = H; io.W = W;
        io.in_format = c.in_format;
        io.in[0] = packed(s->slot[s->prev], c.in_format, H, W);
        io.in[1] = packed(s->slot[cur], c.in_format, H, W);
        io.out_format = c.out_format;
        io.n_t = n_t; io.t = s->t_dev; io.out = outs.data();
        rc = fldr_chroma_forward(s->model, &io, s->ws, s->ws_bytes, stream);
        if (!rc) {
            e = hipMemcpyAsync(out_host, s->out_dev, (size_t)(n_t * s->out_bytes), hipMemcpyDeviceToHost, stream);
            if (e != hipSuccess) rc = (int)e;
        }
    }
    e = hipStreamSynchronize(stream);
    if (!rc && e != hipSuccess) rc = (int)e;
    if (rc) { s->prev = -1; return rc; }                           // the held frame is not to be trusted
    if (interp) {
        for (int k = 0; k < n_t; ++k) copy_planes(host_outs[k], packed(out_host + k * s->out_bytes, c.out_format, H, W), c.out_format, H, W);
        *n_out = n_t;
    }
    s->prev = cur;
    return 0;
}

extern "C" FLDR_CHROMA_API int fldr_chroma_session_reset(fldr_chroma_session* s) {
    if (!s) return FLDR_CHROMA_E_ARG;
    s->prev = -1;
    return 0;
}

extern "C" FLDR_CHROMA_API void fldr_chroma_session_destroy(fldr_chroma_session* s) {
    if (s) { close_stream_mem(s->sm); delete s; }
}
