// libfldr_rate.so, host side: validation, fldr_scene_measure, fldr_rate_forward (measure -> fldr_video_forward -> select) and the rate
// converter for streams of host frames.  The only fldr_* functions called are those of fldr_video.h and fldr_model.h.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <vector>

#include "rate_internal.h"

using namespace fldr_rate_impl;

namespace {

constexpr int64_t ALIGN = 256;
int64_t align_up(int64_t v) { return (v + ALIGN - 1) / ALIGN * ALIGN; }

// ---- the video API's rules for formats and frames (fldr_video_forward applies the same ones) ----------------------------------------
int planes_of(int layout) { return layout == FLDR_VIDEO_NV12 ? 2 : 3; }
bool deep(const fldr_video_format& f) { return f.depth == 10; }

int check_format(const fldr_video_format& f) {
    if ((unsigned)f.layout > 1u || (unsigned)f.matrix > 1u || (unsigned)f.range > 1u) return FLDR_VIDEO_E_FORMAT;
    if (f.depth != 0 && f.depth != 8 && f.depth != 10) return FLDR_VIDEO_E_FORMAT;
    for (int i = 0; i < 4; ++i) if (f.reserved[i]) return FLDR_VIDEO_E_FORMAT;
    return 0;
}

int64_t row_bytes(const fldr_video_format& f, int p, int W) {
    const int64_t cw = (W + 1) / 2, b = deep(f) ? 2 : 1;
    return b * (p == 0 ? W : (f.layout == FLDR_VIDEO_NV12 ? 2 * cw : cw));
}

int rows_of(int p, int H) { return p == 0 ? H : (H + 1) / 2; }

int check_frame(const fldr_video_frame& fr, const fldr_video_format& f, int W) {
    for (int p = 0; p < planes_of(f.layout); ++p) if (!fr.plane[p] || (deep(f) && ((uintptr_t)fr.plane[p] & 1))) return FLDR_VIDEO_E_PLANE;
    for (int p = 0; p < planes_of(f.layout); ++p)
        if (fr.pitch[p] < row_bytes(f, p, W) || (deep(f) && (fr.pitch[p] & 1))) return FLDR_VIDEO_E_PITCH;
    return 0;
}

bool same_format(const fldr_video_format& a, const fldr_video_format& b) {
    return a.layout == b.layout && a.matrix == b.matrix && a.range == b.range && deep(a) == deep(b);
}

// thresholds with the defaults filled in; FLDR_RATE_E_ARG outside 0 .. 1000 or with a reserved word set
int resolve_params(const fldr_scene_params* p, int& sad_pm, int& hist_pm) {
    sad_pm = FLDR_SCENE_SAD_DEFAULT;
    hist_pm = FLDR_SCENE_HIST_DEFAULT;
    if (!p) return 0;
    if (p->sad_permille < 0 || p->sad_permille > 1000 || p->hist_permille < 0 || p->hist_permille > 1000) return FLDR_RATE_E_ARG;
    if (p->reserved[0] || p->reserved[1]) return FLDR_RATE_E_ARG;
    if (p->sad_permille) sad_pm = p->sad_permille;
    if (p->hist_permille) hist_pm = p->hist_permille;
    return 0;
}

int check_measure(int H, int W, const fldr_video_format* fmt, const fldr_video_frame in[2], const fldr_scene_params* p, void* state,
                  int& sad_pm, int& hist_pm) {
    if (!fmt || !in || H < 1 || W < 1) return FLDR_RATE_E_ARG;
    if (((int64_t)W * 2 + 15) / 16 * (int64_t)H > 0x7fffffffll) return FLDR_RATE_E_ARG;      // the kernel counts 16-byte groups in 32 bits
    int rc = resolve_params(p, sad_pm, hist_pm);
    if (!rc) rc = check_format(*fmt);
    for (int f = 0; f < 2 && !rc; ++f) rc = check_frame(in[f], *fmt, W);
    if (rc) return rc;
    if (!state || ((uintptr_t)state & (ALIGN - 1))) return FLDR_RATE_E_STATE;
    return 0;
}

int enqueue_measure(int H, int W, const fldr_video_format& fmt, const fldr_video_frame in[2], int sad_pm, int hist_pm, void* state, hipStream_t s) {
    const int mode = !deep(fmt) ? Y8_BYTE : fmt.layout == FLDR_VIDEO_NV12 ? Y8_P010 : Y8_LOW10;
    return scene_measure(in[0].plane[0], in[0].pitch[0], in[1].plane[0], in[1].pitch[0], H, W, mode, sad_pm, hist_pm, state, s);
}

#define CK(x) do { const int rc_ = (x); if (rc_) return rc_; } while (0)

}  // namespace

extern "C" FLDR_RATE_API int fldr_rate_version(void) { return FLDR_RATE_VERSION; }

extern "C" FLDR_RATE_API const char* fldr_rate_error_string(int code) {
    switch (code) {
    case 0: return "success";
    case FLDR_RATE_E_ARG: return "fldr_rate: bad argument";
    case FLDR_RATE_E_FORMAT: return "fldr_rate: in_format and out_format differ";
    case FLDR_RATE_E_STATE: return "fldr_rate: scene state missing or misaligned";
    case FLDR_RATE_E_RATIO: return "fldr_rate: rate terms not positive, or a ratio outside what the converter takes";
    case FLDR_RATE_E_DEVICE: return "fldr_rate: no such device or out of memory";
    default: return code > -200 ? fldr_video_error_string(code) : "fldr_rate: unknown error";
    }
}

extern "C" FLDR_RATE_API int fldr_rate_sizeof(int which) {
    switch (which) {
    case 0: return (int)sizeof(fldr_scene_params);
    case 1: return (int)sizeof(fldr_scene_result);
    case 2: return (int)sizeof(fldr_rate_config);
    default: return FLDR_RATE_E_ARG;
    }
}

extern "C" FLDR_RATE_API int fldr_scene_measure(int H, int W, const fldr_video_format* fmt, const fldr_video_frame in[2],
                                                const fldr_scene_params* p, void* state, void* stream) {
    int sad_pm, hist_pm;
    CK(check_measure(H, W, fmt, in, p, state, sad_pm, hist_pm));
    return enqueue_measure(H, W, *fmt, in, sad_pm, hist_pm, state, (hipStream_t)stream);
}

extern "C" FLDR_RATE_API int64_t fldr_rate_workspace_bytes(const fldr_model* m, int H, int W, int n_t) {
    const int64_t vb = fldr_video_workspace_bytes(m, H, W, n_t);
    return vb < 0 ? vb : align_up(vb) + FLDR_SCENE_STATE_BYTES;
}

extern "C" FLDR_RATE_API int fldr_rate_forward(const fldr_model* m, const fldr_video_io* io, const fldr_scene_params* p, void* ws, int64_t ws_bytes,
                                               void* stream) {
    // everything fldr_video_forward would refuse is refused here, before the measure is enqueued
    if (!io) return FLDR_RATE_E_ARG;
    if (io->H < 2 || io->W < 2 || io->n_t < 1 || !io->t || !io->out) return FLDR_VIDEO_E_ARG;
    int sad_pm, hist_pm;
    CK(resolve_params(p, sad_pm, hist_pm));
    CK(check_format(io->in_format));
    CK(check_format(io->out_format));
    if (!same_format(io->in_format, io->out_format)) return FLDR_RATE_E_FORMAT;
    const fldr_video_format& fmt = io->in_format;
    for (int f = 0; f < 2; ++f) CK(check_frame(io->in[f], fmt, io->W));
    for (int k = 0; k < io->n_t; ++k) CK(check_frame(io->out[k], fmt, io->W));
    const int64_t vb = fldr_video_workspace_bytes(m, io->H, io->W, io->n_t);
    if (vb < 0) return (int)vb;
    const int64_t state_off = align_up(vb);
    if (!ws || ((uintptr_t)ws & (ALIGN - 1)) || ws_bytes < state_off + FLDR_SCENE_STATE_BYTES) return FLDR_VIDEO_E_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    void* state = (char*)ws + state_off;
    CK(enqueue_measure(io->H, io->W, fmt, io->in, sad_pm, hist_pm, state, s));
    CK(fldr_video_forward(m, io, ws, state_off, stream));
    int64_t rb[3];
    int rows[3];
    const int np = planes_of(fmt.layout);
    for (int q = 0; q < 3; ++q) { rb[q] = q < np ? row_bytes(fmt, q, io->W) : 0; rows[q] = q < np ? rows_of(q, io->H) : 0; }
    for (int k0 = 0; k0 < io->n_t; k0 += SELECT_MAX_OUT) {
        const int n = io->n_t - k0 < SELECT_MAX_OUT ? io->n_t - k0 : SELECT_MAX_OUT;
        CK(select_on_cut(state, io->t + k0, io->in, io->out + k0, n, np, rb, rows, s));
    }
    return 0;
}

// ---- the rate converter ---------------------------------------------------------------------------------------------------------------
struct fldr_rate {
    const fldr_model* model;
    fldr_rate_config cfg;
    int device;
    int64_t A, B;                      // output j at input position j A / B
    int max_out;
    hipStream_t stream;
    char* mem;                         // device: slot 0, slot 1, max_out outputs, t, scene state (pairs without a forward), workspace
    uint8_t* pinned;                   // host: two input frames (the held one and the new one), max_out output frames, t, the scene result
    int64_t frame_bytes, ws_bytes;
    uint8_t* slot[2];
    uint8_t* out_dev;
    float* t_dev;
    void* state_dev;
    void* ws;
    uint8_t* in_host[2];
    uint8_t* out_host;
    float* t_host;
    fldr_scene_result* scene_host;
    int prev;                          // slot holding the previous frame, -1 when none
    int64_t n;                         // frames pushed since create / reset
    int64_t j;                         // the next output frame
};

namespace {

struct DeviceGuard {                                      // make `dev` current, restore the caller's device on exit
    int prev = -1;
    int rc = 0;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev && hipSetDevice(dev) != hipSuccess) rc = FLDR_RATE_E_DEVICE;
    }
    ~DeviceGuard() { if (prev >= 0) { int cur = -1; if (hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev); } }
};

// packed planes of one frame (pitch = row bytes) starting at `base`
fldr_video_frame packed(uint8_t* base, const fldr_video_format& fmt, int H, int W) {
    fldr_video_frame f;
    memset(&f, 0, sizeof(f));
    int64_t off = 0;
    for (int p = 0; p < planes_of(fmt.layout); ++p) {
        f.plane[p] = base + off;
        f.pitch[p] = row_bytes(fmt, p, W);
        off += f.pitch[p] * rows_of(p, H);
    }
    return f;
}

int64_t frame_size(const fldr_video_format& fmt, int H, int W) {
    int64_t n = 0;
    for (int p = 0; p < planes_of(fmt.layout); ++p) n += row_bytes(fmt, p, W) * rows_of(p, H);
    return n;
}

// rows of every plane from `src` (any pitches) to `dst` (any pitches), on the host
void copy_planes(const fldr_video_frame& dst, const fldr_video_frame& src, const fldr_video_format& fmt, int H, int W) {
    for (int p = 0; p < planes_of(fmt.layout); ++p) {
        const int64_t rb = row_bytes(fmt, p, W), n = rows_of(p, H);
        for (int64_t r = 0; r < n; ++r)
            memcpy((uint8_t*)dst.plane[p] + r * dst.pitch[p], (const uint8_t*)src.plane[p] + r * src.pitch[p], (size_t)rb);
    }
}

void release(fldr_rate* s) {
    DeviceGuard g(s->device);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    if (s->mem) (void)hipFree(s->mem);
    if (s->pinned) (void)hipHostFree(s->pinned);
    (void)hipGetLastError();
    delete s;
}

int64_t gcd64(int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; }

}  // namespace

extern "C" FLDR_RATE_API int fldr_rate_create(const fldr_model* m, const fldr_rate_config* cfg, fldr_rate** out) {
    if (!cfg || !out) return FLDR_RATE_E_ARG;
    *out = nullptr;
    if (cfg->H < 2 || cfg->W < 2 || cfg->device < 0 || (unsigned)cfg->scene > 1u) return FLDR_RATE_E_ARG;
    for (int i = 0; i < 4; ++i) if (cfg->reserved[i]) return FLDR_RATE_E_ARG;
    int sad_pm, hist_pm;
    CK(resolve_params(&cfg->scene_params, sad_pm, hist_pm));
    CK(check_format(cfg->format));
    if (cfg->in_num <= 0 || cfg->in_den <= 0 || cfg->out_num <= 0 || cfg->out_den <= 0) return FLDR_RATE_E_RATIO;
    int64_t A = (int64_t)cfg->in_num * cfg->out_den, B = (int64_t)cfg->in_den * cfg->out_num;
    const int64_t g = gcd64(A, B);
    A /= g; B /= g;
    // t = (float)r / (float)B is then exact in its operands, and t < 0.5f exactly where r * 2 < B
    if (A > (1ll << 24) || B > (1ll << 24) || (B + A - 1) / A > FLDR_RATE_MAX_OUT) return FLDR_RATE_E_RATIO;
    const int max_out = (int)((B + A - 1) / A);
    if (!m) return FLDR_RATE_E_ARG;
    const int H = cfg->H, W = cfg->W;
    const int64_t wsb = fldr_rate_workspace_bytes(m, H, W, max_out);
    if (wsb < 0) return (int)wsb;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device >= ndev) { (void)hipGetLastError(); return FLDR_RATE_E_DEVICE; }
    fldr_rate* s = new (std::nothrow) fldr_rate();
    if (!s) return FLDR_RATE_E_DEVICE;
    s->model = m;
    s->cfg = *cfg;
    s->device = cfg->device;
    s->A = A; s->B = B; s->max_out = max_out;
    s->prev = -1; s->n = 0; s->j = 0;
    s->frame_bytes = align_up(frame_size(cfg->format, H, W));
    s->ws_bytes = wsb;
    DeviceGuard guard(s->device);
    if (guard.rc) { delete s; return guard.rc; }
    const int64_t t_bytes = align_up(4ll * max_out);
    const int64_t dev_total = (2 + max_out) * s->frame_bytes + t_bytes + FLDR_SCENE_STATE_BYTES + wsb;
    const int64_t host_total = (2 + max_out) * s->frame_bytes + t_bytes + ALIGN;
    if (hipMalloc((void**)&s->mem, (size_t)dev_total) != hipSuccess) { s->mem = nullptr; release(s); return FLDR_RATE_E_DEVICE; }
    if (hipHostMalloc((void**)&s->pinned, (size_t)host_total, hipHostMallocDefault) != hipSuccess) { s->pinned = nullptr; release(s); return FLDR_RATE_E_DEVICE; }
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) { s->stream = nullptr; release(s); return FLDR_RATE_E_DEVICE; }
    s->slot[0] = (uint8_t*)s->mem;
    s->slot[1] = s->slot[0] + s->frame_bytes;
    s->out_dev = s->slot[1] + s->frame_bytes;
    s->t_dev = (float*)(s->out_dev + max_out * s->frame_bytes);
    s->state_dev = (char*)s->t_dev + t_bytes;
    s->ws = (char*)s->state_dev + FLDR_SCENE_STATE_BYTES;
    s->in_host[0] = s->pinned;
    s->in_host[1] = s->pinned + s->frame_bytes;
    s->out_host = s->in_host[1] + s->frame_bytes;
    s->t_host = (float*)(s->out_host + max_out * s->frame_bytes);
    s->scene_host = (fldr_scene_result*)((char*)s->t_host + t_bytes);
    *out = s;
    return 0;
}

extern "C" FLDR_RATE_API int fldr_rate_max_out(const fldr_rate* s) { return s ? s->max_out : FLDR_RATE_E_ARG; }

extern "C" FLDR_RATE_API int fldr_rate_push(fldr_rate* s, const fldr_video_frame* frame, const fldr_video_frame* host_outs, int* n_out,
                                            fldr_scene_result* scene) {
    if (!s || !frame || !n_out) return FLDR_RATE_E_ARG;
    *n_out = 0;
    if (scene) memset(scene, 0, sizeof(*scene));
    const fldr_rate_config& c = s->cfg;
    const int H = c.H, W = c.W;
    const fldr_video_format& fmt = c.format;
    CK(check_frame(*frame, fmt, W));
    // the outputs of the pair (n - 1, n): every j with (n - 1) B <= j A < n B; r = j A - (n - 1) B
    const bool pair = s->prev >= 0;
    int count = 0, n_t = 0;
    int64_t r_of[FLDR_RATE_MAX_OUT];
    if (pair)
        for (int64_t j = s->j; j * s->A < s->n * s->B && count < FLDR_RATE_MAX_OUT; ++j) {
            r_of[count] = j * s->A - (s->n - 1) * s->B;
            if (r_of[count]) ++n_t;
            ++count;
        }
    if (count) {
        if (!host_outs) return FLDR_RATE_E_ARG;
        for (int k = 0; k < count; ++k) CK(check_frame(host_outs[k], fmt, W));
    }
    DeviceGuard g(s->device);
    if (g.rc) return g.rc;
    const int cur = s->prev == 0 ? 1 : 0;                          // the slot not holding the previous frame
    copy_planes(packed(s->in_host[cur], fmt, H, W), *frame, fmt, H, W);
    hipError_t e = hipMemcpyAsync(s->slot[cur], s->in_host[cur], (size_t)s->frame_bytes, hipMemcpyHostToDevice, s->stream);
    int rc = e == hipSuccess ? 0 : (int)e;
    const bool measure = pair && c.scene == 1;
    if (!rc && pair && (n_t || measure)) {
        fldr_video_frame in[2] = { packed(s->slot[s->prev], fmt, H, W), packed(s->slot[cur], fmt, H, W) };
        void* state = s->state_dev;
        if (n_t) {
            for (int k = 0, q = 0; k < count; ++k) if (r_of[k]) s->t_host[q++] = (float)r_of[k] / (float)s->B;
            e = hipMemcpyAsync(s->t_dev, s->t_host, 4ull * n_t, hipMemcpyHostToDevice, s->stream);
            if (e != hipSuccess) rc = (int)e;
            std::vector<fldr_video_frame> outs((size_t)n_t);
            for (int k = 0; k < n_t; ++k) outs[k] = packed(s->out_dev + k * s->frame_bytes, fmt, H, W);
            fldr_video_io io;
            memset(&io, 0, sizeof(io));
            io.H = H; io.W = W;
            io.in_format = io.out_format = fmt;
            io.in[0] = in[0]; io.in[1] = in[1];
            io.n_t = n_t; io.t = s->t_dev; io.out = outs.data();
            if (!rc && measure) {
                // the forward always runs; on a cut the select of fldr_rate_forward overwrites its outputs on the device
                const int64_t need = fldr_rate_workspace_bytes(s->model, H, W, n_t);
                rc = need < 0 ? (int)need : fldr_rate_forward(s->model, &io, &c.scene_params, s->ws, s->ws_bytes, s->stream);
                state = (char*)s->ws + need - FLDR_SCENE_STATE_BYTES;
            } else if (!rc) {
                rc = fldr_video_forward(s->model, &io, s->ws, s->ws_bytes, s->stream);
            }
            if (!rc) {
                e = hipMemcpyAsync(s->out_host, s->out_dev, (size_t)(n_t * s->frame_bytes), hipMemcpyDeviceToHost, s->stream);
                if (e != hipSuccess) rc = (int)e;
            }
        } else {
            rc = fldr_scene_measure(H, W, &fmt, in, &c.scene_params, state, s->stream);        // a pair without an interpolated output
        }
        if (!rc && measure) {
            e = hipMemcpyAsync(s->scene_host, state, sizeof(fldr_scene_result), hipMemcpyDeviceToHost, s->stream);
            if (e != hipSuccess) rc = (int)e;
        }
    }
    e = hipStreamSynchronize(s->stream);
    if (!rc && e != hipSuccess) rc = (int)e;
    if (rc) { s->prev = -1; s->n = 0; s->j = 0; return rc; }     // the held frame is not to be trusted: as after a reset
    for (int k = 0, q = 0; k < count; ++k) {
        if (r_of[k]) copy_planes(host_outs[k], packed(s->out_host + (q++) * s->frame_bytes, fmt, H, W), fmt, H, W);
        else copy_planes(host_outs[k], packed(s->in_host[s->prev], fmt, H, W), fmt, H, W);                        // frame n - 1, its bytes
    }
    if (measure && scene) *scene = *s->scene_host;
    *n_out = count;
    s->j += count;
    s->n += 1;
    s->prev = cur;
    return 0;
}

extern "C" FLDR_RATE_API int fldr_rate_flush(fldr_rate* s, const fldr_video_frame* host_outs, int* n_out) {
    if (!s || !n_out) return FLDR_RATE_E_ARG;
    *n_out = 0;
    if (s->prev < 0 || s->j * s->A != (s->n - 1) * s->B) return 0;
    if (!host_outs) return FLDR_RATE_E_ARG;
    const fldr_rate_config& c = s->cfg;
    CK(check_frame(host_outs[0], c.format, c.W));
    copy_planes(host_outs[0], packed(s->in_host[s->prev], c.format, c.H, c.W), c.format, c.H, c.W);
    s->j += 1;
    *n_out = 1;
    return 0;
}

extern "C" FLDR_RATE_API int fldr_rate_reset(fldr_rate* s) {
    if (!s) return FLDR_RATE_E_ARG;
    s->prev = -1; s->n = 0; s->j = 0;
    return 0;
}

extern "C" FLDR_RATE_API void fldr_rate_destroy(fldr_rate* s) {
    if (s) release(s);
}
