// libfldr_conform.so, host side: the table (conform_coefs.h), the view, validation, fldr_conform_frame and the stream (host frames in the
// in format and rate in, host frames in the out format, on the canvas, at the out rate out).  The video API's rules for formats and
// frames, the padded frames, the extents of the overlap test and the device / stream / pinned block of a stream object come from
// ../video/frame_host.h; the configuration rules and the schedule of the rate converter from ../rate/rate_plan.h, which includes it; the
// order in which the planes and pitches of a frame are checked from ../rate/tile_measure_host.h.  The only fldr_* functions called are
// those of fldr_rate.h, fldr_video.h and fldr_model.h.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>

#include "../rate/rate_plan.h"
#include "../rate/tile_measure_host.h"
#include "conform_coefs.h"
#include "conform_internal.h"

using namespace fldr_conform_impl;

namespace {

bool size_ok(int v) { return v >= 1 && v <= FLDR_CONFORM_MAX_SIZE; }

// the words every entry shares, in the order fldr_conform.h states: FLDR_RATE_E_ARG, then the formats' FLDR_VIDEO_E_FORMAT
int check_words(int iH, int iW, const fldr_video_format& in_fmt, int oH, int oW, const fldr_video_format& out_fmt, int dst_x, int dst_y, int dither,
                const int32_t* reserved, int n_reserved) {
    if (!size_ok(iH) || !size_ok(iW) || !size_ok(oH) || !size_ok(oW)) return FLDR_RATE_E_ARG;
    if (dst_x < 0 || dst_y < 0 || (dst_x & 1) || (dst_y & 1)) return FLDR_RATE_E_ARG;
    if (dst_x > oW - iW || dst_y > oH - iH) return FLDR_RATE_E_ARG;
    if ((unsigned)dither > (unsigned)FLDR_CONFORM_DITHER_ORDERED) return FLDR_RATE_E_ARG;
    for (int i = 0; i < n_reserved; ++i) if (reserved[i]) return FLDR_RATE_E_ARG;
    CK(check_format(in_fmt));
    return check_format(out_fmt);
}

int lay_of(const fldr_video_format& f) {
    return f.layout == FLDR_VIDEO_NV12 ? (deep(f) ? LAY_P010 : LAY_NV8) : (deep(f) ? LAY_LOW10 : LAY_I8);
}

// any plane of `out` (oH x oW in fo) shares a byte with any plane of `in` (iH x iW in fi)
bool overlaps2(const fldr_video_frame& out, const fldr_video_format& fo, int oH, int oW, const fldr_video_frame& in, const fldr_video_format& fi,
               int iH, int iW) {
    for (int p = 0; p < planes_of(fo.layout); ++p)
        for (int q = 0; q < planes_of(fi.layout); ++q) {
            uintptr_t a0, a1, b0, b1;
            extent(out, fo, p, oH, oW, a0, a1);
            extent(in, fi, q, iH, iW, b0, b1);
            if (a0 < b1 && b0 < a1) return true;
        }
    return false;
}

int check_conform_frame(const fldr_conform_config* c, const fldr_video_frame* in, const fldr_video_frame* out) {
    if (!c || !in || !out) return FLDR_RATE_E_ARG;
    CK(check_words(c->in_H, c->in_W, c->in_format, c->out_H, c->out_W, c->out_format, c->dst_x, c->dst_y, c->dither, c->reserved, 3));
    CK(check_frames(&in, 1, c->in_format, c->in_W));
    CK(check_frames(&out, 1, c->out_format, c->out_W));
    if (overlaps2(*out, c->out_format, c->out_H, c->out_W, *in, c->in_format, c->in_H, c->in_W)) return FLDR_RATE_E_ARG;
    return 0;
}

// the launch of a checked call
int enqueue_conform(const fldr_conform_config& c, const fldr_video_frame& in, const fldr_video_frame& out, hipStream_t stream) {
    ConformArgs a;
    memset(&a, 0, sizeof(a));
    for (int p = 0; p < planes_of(c.in_format.layout); ++p) { a.src[p] = (const uint8_t*)in.plane[p]; a.pitch_src[p] = in.pitch[p]; }
    for (int p = 0; p < planes_of(c.out_format.layout); ++p) { a.dst[p] = (uint8_t*)out.plane[p]; a.pitch_dst[p] = out.pitch[p]; }
    a.in_H = c.in_H; a.in_W = c.in_W; a.out_H = c.out_H; a.out_W = c.out_W;
    a.dst_x = c.dst_x; a.dst_y = c.dst_y;
    int32_t k[7];
    conform_coefs(c.in_format, c.out_format, k);
    a.kyy = k[FLDR_CONFORM_KYY]; a.kyu = k[FLDR_CONFORM_KYU]; a.kyv = k[FLDR_CONFORM_KYV];
    a.kuu = k[FLDR_CONFORM_KUU]; a.kuv = k[FLDR_CONFORM_KUV]; a.kvu = k[FLDR_CONFORM_KVU]; a.kvv = k[FLDR_CONFORM_KVV];
    const ConformSide s = conform_side(c.in_format), d = conform_side(c.out_format);
    a.yo_s = s.yo; a.cc_s = s.cc; a.yo_d = d.yo; a.cc_d = d.cc;
    a.dither = c.dither;
    const int ns = RUN_BYTES / (deep(c.out_format) ? 2 : 1);                                   // samples of a run
    const int cols = c.out_format.layout == FLDR_VIDEO_NV12 ? ns / 2 : ns;                     // chroma columns of a run
    a.luma_runs = (uint32_t)((c.out_W + ns - 1) / ns);
    a.chroma_runs = (uint32_t)(((c.out_W + 1) / 2 + cols - 1) / cols);
    a.luma_blocks = (a.luma_runs * (uint32_t)c.out_H + CONFORM_THREADS - 1) / CONFORM_THREADS;
    a.blocks = a.luma_blocks + (a.chroma_runs * (uint32_t)((c.out_H + 1) / 2) + CONFORM_THREADS - 1) / CONFORM_THREADS;
    return conform(a, lay_of(c.in_format), lay_of(c.out_format), c.in_format.matrix != c.out_format.matrix, stream);
}

}  // namespace

extern "C" FLDR_CONFORM_API int fldr_conform_version(void) { return FLDR_CONFORM_VERSION; }

extern "C" FLDR_CONFORM_API const char* fldr_conform_error_string(int code) { return fldr_rate_error_string(code); }

extern "C" FLDR_CONFORM_API int fldr_conform_sizeof(int which) {
    switch (which) {
    case 0: return (int)sizeof(fldr_conform_config);
    case 1: return (int)sizeof(fldr_conform_stream_config);
    default: return FLDR_RATE_E_ARG;
    }
}

extern "C" FLDR_CONFORM_API int fldr_conform_coefs(const fldr_video_format* src, const fldr_video_format* dst, int32_t coef[7]) {
    if (!src || !dst || !coef) return FLDR_RATE_E_ARG;
    CK(check_format(*src));
    CK(check_format(*dst));
    conform_coefs(*src, *dst, coef);
    return 0;
}

extern "C" FLDR_CONFORM_API int fldr_conform_view(const fldr_video_frame* frame, const fldr_video_format* fmt, int x, int y, fldr_video_frame* view) {
    if (!frame || !fmt || !view) return FLDR_RATE_E_ARG;
    if (x < 0 || y < 0 || (x & 1) || (y & 1)) return FLDR_RATE_E_ARG;
    CK(check_format(*fmt));
    const int np = planes_of(fmt->layout);
    for (int p = 0; p < np; ++p) if (!frame->plane[p]) return FLDR_VIDEO_E_PLANE;
    fldr_video_frame v;
    memset(&v, 0, sizeof(v));
    for (int p = 0; p < np; ++p) {
        // row_bytes of a width is the byte offset of that column in plane p: x is even, so the chroma planes move by x / 2 columns
        v.plane[p] = (uint8_t*)frame->plane[p] + (int64_t)(p ? y / 2 : y) * frame->pitch[p] + row_bytes(*fmt, p, x);
        v.pitch[p] = frame->pitch[p];
    }
    *view = v;
    return 0;
}

extern "C" FLDR_CONFORM_API int fldr_conform_frame(const fldr_conform_config* cfg, const fldr_video_frame* in, const fldr_video_frame* out, void* stream) {
    CK(check_conform_frame(cfg, in, out));
    return enqueue_conform(*cfg, *in, *out, (hipStream_t)stream);
}

// ---- the stream ------------------------------------------------------------------------------------------------------------------------
struct fldr_conform {
    const fldr_model* model;
    fldr_conform_stream_config cfg;
    fldr_conform_config frame_cfg;     // of every conform of the stream
    RatePlan plan;
    bool forwards;
    // device: slot 0, slot 1 (the pushed frames, in the in format), max_out forward outputs (in format), max_out conformed outputs (out
    //         format), t, the scene state of pairs without a forward, the workspace
    // pinned: the frame being pushed, max_out output frames, t, the scene result
    StreamMem sm;
    int64_t slot_bytes, out_bytes, ws_bytes;
    uint8_t* slot[2];
    uint8_t* fwd_out;
    uint8_t* out_dev;
    float* t_dev;
    void* state_dev;
    void* ws;
    uint8_t* in_host;
    uint8_t* out_host;
    float* t_host;
    fldr_scene_result* scene_host;
    int64_t n;                         // frames pushed since create / reset
    int64_t j;                         // the next output frame
};

namespace {

void forget(fldr_conform* s) { s->n = 0; s->j = 0; }

fldr_video_frame slot_frame(const fldr_conform* s, uint8_t* base) { return padded(base, s->cfg.rate.format, s->cfg.rate.H, s->cfg.rate.W); }

fldr_video_frame out_frame(const fldr_conform* s, uint8_t* base) { return padded(base, s->cfg.out_format, s->cfg.out_H, s->cfg.out_W); }

// Output k of a call, which lives at `src` in the in format: conformed, then enqueued to pinned output frame k
int enqueue_output(fldr_conform* s, int k, uint8_t* src) {
    uint8_t* dst = s->out_dev + k * s->out_bytes;
    CK(enqueue_conform(s->frame_cfg, slot_frame(s, src), out_frame(s, dst), s->sm.stream));
    return (int)hipMemcpyAsync(s->out_host + k * s->out_bytes, dst, (size_t)s->out_bytes, hipMemcpyDeviceToHost, s->sm.stream);
}

// the end of a call whose enqueues came to `rc`: the wait, and on success the first `count` pinned output frames go to host_outs
int finish(fldr_conform* s, int rc, const fldr_video_frame* host_outs, int count) {
    const hipError_t e = hipStreamSynchronize(s->sm.stream);
    if (!rc) rc = (int)e;
    if (rc) { (void)hipGetLastError(); forget(s); return rc; }
    const fldr_conform_stream_config& c = s->cfg;
    for (int k = 0; k < count; ++k) copy_planes(host_outs[k], out_frame(s, s->out_host + k * s->out_bytes), c.out_format, c.out_H, c.out_W);
    return 0;
}

}  // namespace

extern "C" FLDR_CONFORM_API int fldr_conform_create(const fldr_model* m, const fldr_conform_stream_config* cfg, fldr_conform** out) {
    if (!cfg || !out) return FLDR_RATE_E_ARG;
    *out = nullptr;
    const fldr_rate_config& r = cfg->rate;
    CK(check_rate_config(r));
    RatePlan plan;
    CK(reduce_rate(r.in_num, r.in_den, r.out_num, r.out_den, plan));
    CK(check_words(r.H, r.W, r.format, cfg->out_H, cfg->out_W, cfg->out_format, cfg->dst_x, cfg->dst_y, cfg->dither, cfg->reserved, 4));
    const bool forwards = plan.B != 1;
    if (forwards && !m) return FLDR_RATE_E_ARG;
    const int64_t wsb = forwards ? fldr_rate_workspace_bytes(m, r.H, r.W, plan.max_out) : 0;
    if (wsb < 0) return (int)wsb;
    if (!device_exists(r.device)) return FLDR_RATE_E_DEVICE;
    fldr_conform* s = new (std::nothrow) fldr_conform();
    if (!s) return FLDR_RATE_E_DEVICE;
    s->model = m;
    s->cfg = *cfg;
    fldr_conform_config& fc = s->frame_cfg;
    memset(&fc, 0, sizeof(fc));
    fc.in_H = r.H; fc.in_W = r.W; fc.in_format = r.format;
    fc.out_H = cfg->out_H; fc.out_W = cfg->out_W; fc.out_format = cfg->out_format;
    fc.dst_x = cfg->dst_x; fc.dst_y = cfg->dst_y; fc.dither = cfg->dither;
    s->plan = plan;
    s->forwards = forwards;
    const int max_out = plan.max_out;
    s->slot_bytes = align_up(padded_bytes(r.format, r.H, r.W));
    s->out_bytes = align_up(padded_bytes(cfg->out_format, cfg->out_H, cfg->out_W));
    s->ws_bytes = wsb;
    const int64_t t_bytes = align_up(4ll * max_out);
    const int64_t fwd_bytes = forwards ? max_out * s->slot_bytes : 0;
    const int64_t dev_total = 2 * s->slot_bytes + fwd_bytes + max_out * s->out_bytes + t_bytes + FLDR_SCENE_STATE_BYTES + wsb;
    const int64_t host_total = s->slot_bytes + max_out * s->out_bytes + t_bytes + ALIGN;
    if (!open_stream_mem(s->sm, r.device, dev_total, host_total)) {
        delete s;
        return FLDR_RATE_E_DEVICE;
    }
    s->slot[0] = s->sm.dev;
    s->slot[1] = s->slot[0] + s->slot_bytes;
    s->fwd_out = s->slot[1] + s->slot_bytes;
    s->out_dev = s->fwd_out + fwd_bytes;
    s->t_dev = (float*)(s->out_dev + max_out * s->out_bytes);
    s->state_dev = (uint8_t*)s->t_dev + t_bytes;
    s->ws = forwards ? (uint8_t*)s->state_dev + FLDR_SCENE_STATE_BYTES : nullptr;
    s->in_host = s->sm.pinned;
    s->out_host = s->in_host + s->slot_bytes;
    s->t_host = (float*)(s->out_host + max_out * s->out_bytes);
    s->scene_host = (fldr_scene_result*)((uint8_t*)s->t_host + t_bytes);
    forget(s);
    *out = s;
    return 0;
}

extern "C" FLDR_CONFORM_API int fldr_conform_max_out(const fldr_conform* s) { return s ? s->plan.max_out : FLDR_RATE_E_ARG; }

extern "C" FLDR_CONFORM_API int fldr_conform_push(fldr_conform* s, const fldr_video_frame* frame, const fldr_video_frame* host_outs, int* n_out,
                                                  fldr_scene_result* scene) {
    if (!s || !frame || !n_out) return FLDR_RATE_E_ARG;
    *n_out = 0;
    if (scene) memset(scene, 0, sizeof(*scene));
    const fldr_conform_stream_config& c = s->cfg;
    const fldr_rate_config& r = c.rate;
    const fldr_video_format& fmt = r.format;
    CK(check_frame(*frame, fmt, r.W));
    const bool pair = s->n >= 1;
    int n_t = 0;
    int64_t r_of[FLDR_RATE_MAX_OUT];
    const int count = pair ? pair_outputs(s->plan, s->n, s->j, r_of, n_t) : 0;
    if (count) {
        if (!host_outs) return FLDR_RATE_E_ARG;
        for (int k = 0; k < count; ++k) CK(check_frame(host_outs[k], c.out_format, c.out_W));
    }
    DeviceGuard g(s->sm.device);
    if (!g.ok) return FLDR_RATE_E_DEVICE;
    const hipStream_t stream = s->sm.stream;
    uint8_t* cur = s->slot[s->n & 1];
    uint8_t* prev = s->slot[(s->n - 1) & 1];
    copy_planes(padded(s->in_host, fmt, r.H, r.W), *frame, fmt, r.H, r.W);
    int rc = (int)hipMemcpyAsync(cur, s->in_host, (size_t)s->slot_bytes, hipMemcpyHostToDevice, stream);
    const bool measure = pair && r.scene == 1;
    if (!rc && (n_t || measure)) {
        fldr_video_io io;
        memset(&io, 0, sizeof(io));
        io.H = r.H; io.W = r.W;
        io.in_format = io.out_format = fmt;
        io.in[0] = slot_frame(s, prev); io.in[1] = slot_frame(s, cur);
        void* state = s->state_dev;
        if (n_t) {
            fill_times(r_of, count, s->plan.B, s->t_host);
            rc = (int)hipMemcpyAsync(s->t_dev, s->t_host, 4ull * n_t, hipMemcpyHostToDevice, stream);
            fldr_video_frame outs[FLDR_RATE_MAX_OUT];
            for (int q = 0; q < n_t; ++q) outs[q] = slot_frame(s, s->fwd_out + q * s->slot_bytes);
            io.n_t = n_t; io.t = s->t_dev; io.out = outs;
            if (!rc && measure) {
                // the forward always runs; on a cut the select of fldr_rate_forward overwrites its outputs on the device
                const int64_t need = fldr_rate_workspace_bytes(s->model, r.H, r.W, n_t);
                rc = need < 0 ? (int)need : fldr_rate_forward(s->model, &io, &r.scene_params, s->ws, s->ws_bytes, stream);
                state = (uint8_t*)s->ws + need - FLDR_SCENE_STATE_BYTES;
            } else if (!rc) {
                rc = fldr_video_forward(s->model, &io, s->ws, s->ws_bytes, stream);
            }
        } else {
            rc = fldr_scene_measure(r.H, r.W, &fmt, io.in, &r.scene_params, state, stream);          // a pair without an interpolated output
        }
        if (!rc && measure) rc = (int)hipMemcpyAsync(s->scene_host, state, sizeof(fldr_scene_result), hipMemcpyDeviceToHost, stream);
    }
    for (int k = 0, q = 0; k < count && !rc; ++k) rc = enqueue_output(s, k, r_of[k] ? s->fwd_out + (q++) * s->slot_bytes : prev);
    rc = finish(s, rc, host_outs, count);
    if (rc) return rc;
    if (measure && scene) *scene = *s->scene_host;
    *n_out = count;
    s->j += count;
    s->n += 1;
    return 0;
}

extern "C" FLDR_CONFORM_API int fldr_conform_flush(fldr_conform* s, const fldr_video_frame* host_outs, int* n_out) {
    if (!s || !n_out) return FLDR_RATE_E_ARG;
    *n_out = 0;
    if (!s->n || !flush_due(s->plan, s->n, s->j)) return 0;
    if (!host_outs) return FLDR_RATE_E_ARG;
    CK(check_frame(host_outs[0], s->cfg.out_format, s->cfg.out_W));
    DeviceGuard g(s->sm.device);
    if (!g.ok) return FLDR_RATE_E_DEVICE;
    int rc = enqueue_output(s, 0, s->slot[(s->n - 1) & 1]);
    rc = finish(s, rc, host_outs, 1);
    if (rc) return rc;
    s->j += 1;
    *n_out = 1;
    return 0;
}

extern "C" FLDR_CONFORM_API int fldr_conform_reset(fldr_conform* s) {
    if (!s) return FLDR_RATE_E_ARG;
    forget(s);
    return 0;
}

extern "C" FLDR_CONFORM_API void fldr_conform_destroy(fldr_conform* s) {
    if (!s) return;
    close_stream_mem(s->sm);
    delete s;
}
