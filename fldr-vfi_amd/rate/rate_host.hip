// libfldr_rate.so, host side: validation, fldr_scene_measure, fldr_rate_forward (measure -> fldr_video_forward -> select) and the rate
// converter for streams of host frames.  The video API's rules for formats and frames, and the stream / device block / pinned block the
// converter owns, come from ../video/frame_host.h; the converter's configuration rules, its schedule and the device work of a pair from
// rate_plan.h, which the pipe and cadence libraries compile too.  The only fldr_* functions called are those of fldr_video.h and fldr_model.h.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>

#include "rate_internal.h"
#include "rate_plan.h"

using namespace fldr_rate_impl;

namespace {

bool same_format(const fldr_video_format& a, const fldr_video_format& b) {
    return a.layout == b.layout && a.matrix == b.matrix && a.range == b.range && deep(a) == deep(b);
}

// thresholds with the defaults filled in; check_scene_params' code for those it refuses
int resolve_params(const fldr_scene_params* p, int& sad_pm, int& hist_pm) {
    sad_pm = FLDR_SCENE_SAD_DEFAULT;
    hist_pm = FLDR_SCENE_HIST_DEFAULT;
    if (!p) return 0;
    CK(check_scene_params(*p));
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
    return scene_measure(in[0].plane[0], in[0].pitch[0], in[1].plane[0], in[1].pitch[0], H, W, luma_mode(deep(fmt), fmt.layout), sad_pm, hist_pm,
                         state, s);
}

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
    RatePlan plan;
    // device: slot 0, slot 1, max_out outputs, t, scene state (pairs without a forward), workspace
    // pinned: two input frames (the held one and the new one), max_out output frames, t, the scene result
    StreamMem sm;
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

extern "C" FLDR_RATE_API int fldr_rate_create(const fldr_model* m, const fldr_rate_config* cfg, fldr_rate** out) {
    if (!cfg || !out) return FLDR_RATE_E_ARG;
    *out = nullptr;
    CK(check_rate_config(*cfg));
    RatePlan plan;
    CK(reduce_rate(cfg->in_num, cfg->in_den, cfg->out_num, cfg->out_den, plan));
    const int max_out = plan.max_out;
    if (!m) return FLDR_RATE_E_ARG;
    const int H = cfg->H, W = cfg->W;
    const int64_t wsb = fldr_rate_workspace_bytes(m, H, W, max_out);
    if (wsb < 0) return (int)wsb;
    if (!device_exists(cfg->device)) return FLDR_RATE_E_DEVICE;
    fldr_rate* s = new (std::nothrow) fldr_rate();
    if (!s) return FLDR_RATE_E_DEVICE;
    s->model = m;
    s->cfg = *cfg;
    s->plan = plan;
    s->prev = -1; s->n = 0; s->j = 0;
    s->frame_bytes = align_up(packed_bytes(cfg->format, H, W));
    s->ws_bytes = wsb;
    const int64_t t_bytes = align_up(4ll * max_out);
    const int64_t dev_total = (2 + max_out) * s->frame_bytes + t_bytes + FLDR_SCENE_STATE_BYTES + wsb;
    const int64_t host_total = (2 + max_out) * s->frame_bytes + t_bytes + ALIGN;
    if (!open_stream_mem(s->sm, cfg->device, dev_total, host_total)) { delete s; return FLDR_RATE_E_DEVICE; }
    s->slot[0] = s->sm.dev;
    s->slot[1] = s->slot[0] + s->frame_bytes;
    s->out_dev = s->slot[1] + s->frame_bytes;
    s->t_dev = (float*)(s->out_dev + max_out * s->frame_bytes);
    s->state_dev = (char*)s->t_dev + t_bytes;
    s->ws = (char*)s->state_dev + FLDR_SCENE_STATE_BYTES;
    s->in_host[0] = s->sm.pinned;
    s->in_host[1] = s->in_host[0] + s->frame_bytes;
    s->out_host = s->in_host[1] + s->frame_bytes;
    s->t_host = (float*)(s->out_host + max_out * s->frame_bytes);
    s->scene_host = (fldr_scene_result*)((char*)s->t_host + t_bytes);
    *out = s;
    return 0;
}

extern "C" FLDR_RATE_API int fldr_rate_max_out(const fldr_rate* s) { return s ? s->plan.max_out : FLDR_RATE_E_ARG; }

extern "C" FLDR_RATE_API int fldr_rate_push(fldr_rate* s, const fldr_video_frame* frame, const fldr_video_frame* host_outs, int* n_out,
                                            fldr_scene_result* scene) {
    if (!s || !frame || !n_out) return FLDR_RATE_E_ARG;
    *n_out = 0;
    if (scene) memset(scene, 0, sizeof(*scene));
    const fldr_rate_config& c = s->cfg;
    const int H = c.H, W = c.W;
    const fldr_video_format& fmt = c.format;
    CK(check_frame(*frame, fmt, W));
    const bool pair = s->prev >= 0;
    int n_t = 0;
    int64_t r_of[FLDR_RATE_MAX_OUT];
    const int count = pair ? pair_outputs(s->plan, s->n, s->j, r_of, n_t) : 0;
    if (count) {
        if (!host_outs) return FLDR_RATE_E_ARG;
        for (int k = 0; k < count; ++k) CK(check_frame(host_outs[k], fmt, W));
    }
    DeviceGuard g(s->sm.device);
    if (!g.ok) return FLDR_RATE_E_DEVICE;
    const hipStream_t stream = s->sm.stream;
    const int cur = s->prev == 0 ? 1 : 0;                          // the slot not holding the previous frame
    hipError_t e = upload_frame(s->sm, s->slot[cur], s->in_host[cur], s->frame_bytes, *frame, fmt, H, W);
    int rc = e == hipSuccess ? 0 : (int)e;
    const bool measure = pair && c.scene == 1;
    if (!rc && pair && (n_t || measure)) {
        if (n_t) {
            fill_times(r_of, count, s->plan.B, s->t_host);
            e = hipMemcpyAsync(s->t_dev, s->t_host, 4ull * n_t, hipMemcpyHostToDevice, stream);
            if (e != hipSuccess) rc = (int)e;
        }
        if (!rc) rc = enqueue_pair(s->model, c, n_t, s->slot[s->prev], s->slot[cur], s->out_dev, s->frame_bytes, s->t_dev, s->ws, s->ws_bytes,
                                   s->state_dev, s->scene_host, stream);
        if (!rc && n_t) {
            e = hipMemcpyAsync(s->out_host, s->out_dev, (size_t)(n_t * s->frame_bytes), hipMemcpyDeviceToHost, stream);
            if (e != hipSuccess) rc = (int)e;
        }
    }
    e = hipStreamSynchronize(stream);
    if (!rc && e != hipSuccess) rc = (int)e;
    if (rc) { s->prev = -1; s->n = 0; s->j = 0; return rc; }     // the held frame is not to be trusted: as after a reset
    for (int k = 0, q = 0; k < count; ++k) {
        if (r_of[k]) unpack_frame(host_outs[k], s->out_host + (q++) * s->frame_bytes, fmt, H, W);
        else unpack_frame(host_outs[k], s->in_host[s->prev], fmt, H, W);                                          // frame n - 1, its bytes
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
    if (s->prev < 0 || !flush_due(s->plan, s->n, s->j)) return 0;
    if (!host_outs) return FLDR_RATE_E_ARG;
    const fldr_rate_config& c = s->cfg;
    CK(check_frame(host_outs[0], c.format, c.W));
    unpack_frame(host_outs[0], s->in_host[s->prev], c.format, c.H, c.W);
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
    if (s) { close_stream_mem(s->sm); delete s; }
}
