// libfldr_field.so, host side: validation, fldr_field_weave, fldr_field_forward (measure -> t -> fldr_video_forward on the field views ->
// weave), the schedule and the stream (woven host frames in, progressive host frames out).  The video API's rules for formats and
// frames, and the slots, the pinned frames and the two ends of a stream call (PaddedStream), come from ../video/frame_host.h; the rule
// of the cut thresholds from ../rate/rate_plan.h, which includes it; the fill of a plane's walk from ../video/weave_walk_host.h.  The
// only fldr_* functions called are those of fldr_rate.h, fldr_video.h and fldr_model.h.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>

#include "../rate/rate_plan.h"
#include "../video/weave_walk_host.h"
#include "field_internal.h"

using namespace fldr_field_impl;

namespace {

constexpr int64_t T_BYTES = ALIGN;                                     // the t word has a line of its own
constexpr uint32_t HALF_F32 = 0x3f000000u;                             // 0.5f

int max_code(const fldr_video_format& f) { return deep(f) ? 1023 : 255; }

// still and slack with the defaults filled in; FLDR_FIELD_E_ARG out of range or with a reserved word set
int resolve_params(const fldr_field_params* p, const fldr_video_format& f, int& still, int& slack) {
    const int up = deep(f) ? 2 : 0;
    still = FLDR_FIELD_STILL_DEFAULT8 << up;
    slack = FLDR_FIELD_SLACK_DEFAULT8 << up;
    if (!p) return 0;
    if (p->still < -1 || p->still > max_code(f) || p->slack < 0 || p->slack > max_code(f)) return FLDR_FIELD_E_ARG;
    if (p->reserved[0] || p->reserved[1]) return FLDR_FIELD_E_ARG;
    still = p->still; slack = p->slack;
    return 0;
}

// the field of parity `par` of a frame: H / 2 x W, no copy
fldr_video_frame field_view(const fldr_video_frame& fr, const fldr_video_format& f, int par) {
    fldr_video_frame v;
    memset(&v, 0, sizeof(v));
    for (int p = 0; p < planes_of(f.layout); ++p) {
        v.plane[p] = (uint8_t*)fr.plane[p] + par * fr.pitch[p];
        v.pitch[p] = 2 * fr.pitch[p];
    }
    return v;
}

// the launch arguments of a checked call; false for a frame beyond the kernel's index arithmetic (fldr_field.h: FLDR_FIELD_E_ARG)
bool weave_args(int H, int W, const fldr_video_format& f, const fldr_video_frame& cur, const fldr_video_frame* prev, const fldr_video_frame* next,
                const fldr_video_frame* temporal, int parity, bool intra, const uint32_t* intra_if, int still, int slack,
                const fldr_video_frame& out, WeaveArgs& a) {
    memset(&a, 0, sizeof(a));
    a.planes = planes_of(f.layout);
    a.parity = parity;
    a.intra = intra ? 1 : 0;
    a.intra_if = intra_if;
    a.still = still; a.slack = slack;
    int64_t total = 0;
    for (int p = 0; p < a.planes; ++p) {
        WeavePlane& q = a.pl[p];
        // one work item per group and own row, and the limit is judged on the own rows too (fldr_field.h)
        const int64_t own_rows = rows_of(p, H) / 2;
        if (!fill_walk(q, f, p, H, W, out, own_rows, own_rows, total)) return false;
        q.cur = (const uint8_t*)cur.plane[p]; q.pitch_cur = cur.pitch[p];
        bool vec = aligned16(q.cur, q.pitch_cur) && aligned16(q.out, q.pitch_out);
        if (!intra) {
            q.prev = (const uint8_t*)prev->plane[p]; q.pitch_prev = prev->pitch[p];
            q.next = (const uint8_t*)next->plane[p]; q.pitch_next = next->pitch[p];
            q.temporal = (const uint8_t*)temporal->plane[p]; q.pitch_temporal = temporal->pitch[p];
            vec = vec && aligned16(q.prev, q.pitch_prev) && aligned16(q.next, q.pitch_next) && aligned16(q.temporal, q.pitch_temporal);
        }
        q.vec = vec ? 1 : 0;
        q.comp = f.layout == FLDR_VIDEO_NV12 && p == 1 ? 2 : 1;
    }
    a.total = (uint32_t)total;
    return true;
}

int check_weave(int H, int W, const fldr_video_format* fmt, const fldr_video_frame* cur, const fldr_video_frame* prev, const fldr_video_frame* next,
                const fldr_video_frame* temporal, int parity, int mode, const fldr_field_params* p, const fldr_video_frame* out, int& still,
                int& slack) {
    if (!fmt || !cur || !out) return FLDR_FIELD_E_ARG;
    if (!size_ok(H)) return FLDR_FIELD_E_SIZE;
    if (W < 1 || (unsigned)parity > 1u || (unsigned)mode > 1u) return FLDR_FIELD_E_ARG;
    if (mode == FLDR_FIELD_MOTION && (!prev || !next || !temporal)) return FLDR_FIELD_E_ARG;
    CK(check_format(*fmt));
    CK(resolve_params(p, *fmt, still, slack));
    CK(check_frame(*cur, *fmt, W));
    CK(check_frame(*out, *fmt, W));
    if (mode == FLDR_FIELD_MOTION) {
        CK(check_frame(*prev, *fmt, W));
        CK(check_frame(*next, *fmt, W));
        CK(check_frame(*temporal, *fmt, W));
    }
    return 0;
}

// ---- the workspace of a forward: the video forward's, the scene state, the t word, the temporal frame ------------------------------
struct FieldWs { int64_t state, t, temporal, total; };

// the temporal frame: H / 2 x W, every pitch the row bytes aligned up
constexpr int64_t TEMPORAL_PITCH = ALIGN;

int64_t plan_ws(const fldr_model* m, int H, int W, FieldWs& ws) {
    if (!size_ok(H)) return FLDR_FIELD_E_SIZE;
    if (W < 2 || !m) return FLDR_FIELD_E_ARG;
    const int64_t vb = fldr_video_workspace_bytes(m, H / 2, W, 1);
    if (vb < 0) return vb;
    fldr_video_format largest;                                         // yuv420p10le: three planes of 16-bit words
    memset(&largest, 0, sizeof(largest));
    largest.layout = FLDR_VIDEO_I420; largest.depth = 10;
    ws.state = align_up(vb);
    ws.t = ws.state + FLDR_SCENE_STATE_BYTES;
    ws.temporal = ws.t + T_BYTES;
    ws.total = ws.temporal + laid_out_bytes(largest, H / 2, W, TEMPORAL_PITCH);
    return ws.total;
}

fldr_video_frame temporal_frame(uint8_t* base, const fldr_video_format& f, int H, int W) { return laid_out(base, f, H / 2, W, TEMPORAL_PITCH); }

bool tff_rate_ok(const fldr_field_config& c) { return (unsigned)c.tff <= 1u && (c.rate == 1 || c.rate == 2); }

void schedule_of(const fldr_field_config& c, int64_t j, fldr_field_schedule& s) {
    const int64_t m = c.rate == 2 ? j : 2 * j;
    s.field = m;
    s.cur = m >> 1;
    s.prev = m ? (m - 1) >> 1 : -1;
    s.next = (m + 1) >> 1;
    s.parity = (int32_t)((m & 1) ^ (c.tff ? 0 : 1));
    s.reserved = 0;
}

}  // namespace

extern "C" FLDR_FIELD_API int fldr_field_version(void) { return FLDR_FIELD_VERSION; }

extern "C" FLDR_FIELD_API const char* fldr_field_error_string(int code) {
    switch (code) {
    case FLDR_FIELD_E_ARG: return "fldr_field: bad argument";
    case FLDR_FIELD_E_SIZE: return "fldr_field: frame height below 4 or not a multiple of 4";
    case FLDR_FIELD_E_WORKSPACE: return "fldr_field: workspace missing, misaligned or too small";
    case FLDR_FIELD_E_DEVICE: return "fldr_field: no such device or out of memory";
    // above -300: the rate, video and model ranges and hipError_t, which this library passes through.  -300 .. -999 belong to
    // libraries this one never calls: such a code cannot come from here and is answered as unknown.
    default: return code > -300 ? fldr_rate_error_string(code) : "fldr_field: unknown error";
    }
}

extern "C" FLDR_FIELD_API int fldr_field_sizeof(int which) {
    switch (which) {
    case 0: return (int)sizeof(fldr_field_params);
    case 1: return (int)sizeof(fldr_field_io);
    case 2: return (int)sizeof(fldr_field_config);
    case 3: return (int)sizeof(fldr_field_schedule);
    case 4: return (int)sizeof(fldr_field_report);
    default: return FLDR_FIELD_E_ARG;
    }
}

extern "C" FLDR_FIELD_API int fldr_field_weave(int H, int W, const fldr_video_format* fmt, const fldr_video_frame* cur, const fldr_video_frame* prev,
                                               const fldr_video_frame* next, const fldr_video_frame* temporal, int parity, int mode,
                                               const uint32_t* intra_if, const fldr_field_params* p, const fldr_video_frame* out, void* stream) {
    int still, slack;
    CK(check_weave(H, W, fmt, cur, prev, next, temporal, parity, mode, p, out, still, slack));
    WeaveArgs a;
    if (!weave_args(H, W, *fmt, *cur, prev, next, temporal, parity, mode == FLDR_FIELD_INTRA, intra_if, still, slack, *out, a)) return FLDR_FIELD_E_ARG;
    return weave(a, luma_mode(deep(*fmt), fmt->layout), (hipStream_t)stream);
}

extern "C" FLDR_FIELD_API int64_t fldr_field_workspace_bytes(const fldr_model* m, int H, int W) {
    FieldWs ws;
    return plan_ws(m, H, W, ws);
}

extern "C" FLDR_FIELD_API int fldr_field_temporal(const fldr_model* m, int H, int W, const fldr_video_format* fmt, void* ws, fldr_video_frame* frame) {
    if (!fmt || !frame) return FLDR_FIELD_E_ARG;
    FieldWs lay;
    const int64_t total = plan_ws(m, H, W, lay);
    if (total < 0) return (int)total;
    CK(check_format(*fmt));
    if (!ws || ((uintptr_t)ws & (ALIGN - 1))) return FLDR_FIELD_E_WORKSPACE;
    *frame = temporal_frame((uint8_t*)ws + lay.temporal, *fmt, H, W);
    return 0;
}

extern "C" FLDR_FIELD_API void* fldr_field_scene_state(const fldr_model* m, int H, int W, void* ws) {
    FieldWs lay;
    if (!ws || plan_ws(m, H, W, lay) < 0) return nullptr;
    return (uint8_t*)ws + lay.state;
}

extern "C" FLDR_FIELD_API int fldr_field_forward(const fldr_model* m, const fldr_field_io* io, void* ws, int64_t ws_bytes, void* stream) {
    if (!io) return FLDR_FIELD_E_ARG;
    const int H = io->H, W = io->W;
    if (!size_ok(H)) return FLDR_FIELD_E_SIZE;
    if (W < 2 || (unsigned)io->parity > 1u || (unsigned)io->scene > 1u) return FLDR_FIELD_E_ARG;
    for (int i = 0; i < 4; ++i) if (io->reserved[i]) return FLDR_FIELD_E_ARG;
    const fldr_video_format& fmt = io->format;
    CK(check_format(fmt));
    int still, slack;
    CK(resolve_params(io->params, fmt, still, slack));
    CK(check_scene_params(io->scene_params));
    CK(check_frame(io->cur, fmt, W));
    CK(check_frame(io->prev, fmt, W));
    CK(check_frame(io->next, fmt, W));
    CK(check_frame(io->out, fmt, W));
    if (!m) return FLDR_FIELD_E_ARG;
    FieldWs lay;
    const int64_t total = plan_ws(m, H, W, lay);
    if (total < 0) return (int)total;
    if (!ws || ((uintptr_t)ws & (ALIGN - 1)) || ws_bytes < total) return FLDR_FIELD_E_WORKSPACE;
    uint8_t* w = (uint8_t*)ws;
    void* state = w + lay.state;
    float* t_dev = (float*)(w + lay.t);
    const fldr_video_frame temporal = temporal_frame(w + lay.temporal, fmt, H, W);
    const uint32_t* intra_if = io->scene ? &((const fldr_scene_result*)state)->cut : nullptr;
    WeaveArgs a;
    if (!weave_args(H, W, fmt, io->cur, &io->prev, &io->next, &temporal, io->parity, false, intra_if, still, slack, io->out, a)) return FLDR_FIELD_E_ARG;
    // the fields before and after: the rows of the other parity of prev and next
    const fldr_video_frame in[2] = { field_view(io->prev, fmt, 1 - io->parity), field_view(io->next, fmt, 1 - io->parity) };
    const hipStream_t s = (hipStream_t)stream;
    if (io->scene) CK(fldr_scene_measure(H / 2, W, &fmt, in, &io->scene_params, state, stream));
    CK((int)hipMemsetD32Async((hipDeviceptr_t)t_dev, (int)HALF_F32, 1, s));
    fldr_video_io vio;
    memset(&vio, 0, sizeof(vio));
    vio.H = H / 2; vio.W = W;
    vio.in_format = vio.out_format = fmt;
    vio.in[0] = in[0]; vio.in[1] = in[1];
    vio.n_t = 1; vio.t = t_dev; vio.out = &temporal;
    CK(fldr_video_forward(m, &vio, ws, lay.state, stream));
    return weave(a, luma_mode(deep(fmt), fmt.layout), s);
}

extern "C" FLDR_FIELD_API int fldr_field_plan(const fldr_field_config* cfg, int64_t j, fldr_field_schedule* plan) {
    if (!cfg || !plan || !tff_rate_ok(*cfg) || j < 0 || j > (1ll << 61)) return FLDR_FIELD_E_ARG;
    schedule_of(*cfg, j, *plan);
    return 0;
}

// ---- the stream ------------------------------------------------------------------------------------------------------------------------
struct fldr_field {
    const fldr_model* model;
    fldr_field_config cfg;
    fldr_field_params params;
    bool has_params;
    // device, behind the slots: `rate` outputs, the workspace; pinned, behind the `rate` output frames: `rate` scene results
    PaddedStream ps;
    int64_t ws_bytes;
    uint8_t* out_dev;
    void* ws;
    fldr_scene_result* scene_host;
    int64_t n;                         // frames pushed since create / reset
    int64_t j;                         // the next output
};

namespace {

void forget(fldr_field* f) { f->n = 0; f->j = 0; }

const fldr_field_params* params_of(const fldr_field* f) { return f->has_params ? &f->params : nullptr; }

// output k of a call: field s.field woven into the k-th device output; INTRA without a forward when `intra`
int enqueue_output(fldr_field* f, const fldr_field_schedule& s, bool intra, int k) {
    const fldr_field_config& c = f->cfg;
    const PaddedStream& ps = f->ps;
    const hipStream_t stream = ps.sm.stream;
    const fldr_video_frame cur = padded_at(ps, ps.slot[s.cur & 1]);
    const fldr_video_frame out = padded_at(ps, f->out_dev + k * ps.frame_bytes);
    memset(&f->scene_host[k], 0, sizeof(fldr_scene_result));
    if (intra)
        return fldr_field_weave(c.H, c.W, &c.format, &cur, nullptr, nullptr, nullptr, s.parity, FLDR_FIELD_INTRA, nullptr, params_of(f), &out, stream);
    fldr_field_io io;
    memset(&io, 0, sizeof(io));
    io.H = c.H; io.W = c.W;
    io.format = c.format;
    io.cur = cur;
    io.prev = padded_at(ps, ps.slot[s.prev & 1]);
    io.next = padded_at(ps, ps.slot[s.next & 1]);
    io.parity = s.parity;
    io.scene = c.scene;
    io.scene_params = c.scene_params;
    io.params = params_of(f);
    io.out = out;
    CK(fldr_field_forward(f->model, &io, f->ws, f->ws_bytes, stream));
    if (!c.scene) return 0;
    return (int)hipMemcpyAsync(&f->scene_host[k], fldr_field_scene_state(f->model, c.H, c.W, f->ws), sizeof(fldr_scene_result), hipMemcpyDeviceToHost,
                               stream);
}

// copy `count` outputs back in one piece, wait, hand them out; on a failure the object has been reset
int finish(fldr_field* f, int rc, int count, const fldr_field_schedule* s, const bool* intra, const fldr_video_frame* host_outs, int* n_out,
           fldr_field_report* reports) {
    const uint8_t* const from = f->out_dev;
    rc = deliver(f->ps, rc, &from, count ? 1 : 0, count * f->ps.frame_bytes, host_outs, count);
    if (rc) { forget(f); return rc; }
    for (int k = 0; k < count && reports; ++k) {
        fldr_field_report& r = reports[k];
        memset(&r, 0, sizeof(r));
        r.field = s[k].field;
        r.parity = (uint32_t)s[k].parity;
        r.scene = f->scene_host[k];
        r.cut = r.scene.cut;
        r.mode_used = intra[k] || r.cut ? FLDR_FIELD_INTRA : FLDR_FIELD_MOTION;
    }
    *n_out = count;
    f->j += count;
    return 0;
}

}  // namespace

extern "C" FLDR_FIELD_API int fldr_field_create(const fldr_model* m, const fldr_field_config* cfg, fldr_field** out) {
    if (!cfg || !out) return FLDR_FIELD_E_ARG;
    *out = nullptr;
    if (!size_ok(cfg->H)) return FLDR_FIELD_E_SIZE;
    if (cfg->W < 2 || !tff_rate_ok(*cfg) || cfg->device < 0 || (unsigned)cfg->scene > 1u) return FLDR_FIELD_E_ARG;
    for (int i = 0; i < 4; ++i) if (cfg->reserved[i]) return FLDR_FIELD_E_ARG;
    CK(check_format(cfg->format));
    int still, slack;
    CK(resolve_params(cfg->params, cfg->format, still, slack));
    CK(check_scene_params(cfg->scene_params));
    if (!m) return FLDR_FIELD_E_ARG;
    const int H = cfg->H, W = cfg->W, rate = cfg->rate;
    const int64_t wsb = fldr_field_workspace_bytes(m, H, W);
    if (wsb < 0) return (int)wsb;
    if (!device_exists(cfg->device)) return FLDR_FIELD_E_DEVICE;
    fldr_field* f = new (std::nothrow) fldr_field();
    if (!f) return FLDR_FIELD_E_DEVICE;
    f->model = m;
    f->cfg = *cfg;
    f->has_params = cfg->params != nullptr;
    if (f->has_params) f->params = *cfg->params;
    f->cfg.params = nullptr;
    f->ws_bytes = wsb;
    if (!open_padded_stream(f->ps, cfg->device, cfg->format, H, W, rate, wsb, rate, align_up(rate * (int64_t)sizeof(fldr_scene_result)))) {
        delete f;
        return FLDR_FIELD_E_DEVICE;
    }
    f->out_dev = f->ps.dev_rest;
    f->ws = f->out_dev + rate * f->ps.frame_bytes;
    f->scene_host = (fldr_scene_result*)(f->ps.out_host + rate * f->ps.frame_bytes);
    forget(f);
    *out = f;
    return 0;
}

extern "C" FLDR_FIELD_API int fldr_field_max_out(const fldr_field* f) { return f ? f->cfg.rate : FLDR_FIELD_E_ARG; }

extern "C" FLDR_FIELD_API int fldr_field_push(fldr_field* f, const fldr_video_frame* frame, const fldr_video_frame* host_outs, int* n_out,
                                              fldr_field_report* reports) {
    if (!f || !frame || !n_out) return FLDR_FIELD_E_ARG;
    *n_out = 0;
    const fldr_field_config& c = f->cfg;
    CK(check_frame(*frame, c.format, c.W));
    // every output whose field m + 1 is in a frame pushed by now: at most `rate` of them
    fldr_field_schedule s[2];
    bool intra[2];
    int count = 0;
    for (; count < c.rate; ++count) {
        schedule_of(c, f->j + count, s[count]);
        if (s[count].next > f->n) break;
        intra[count] = s[count].prev < 0;
    }
    CK(check_outs(f->ps, host_outs, count, FLDR_FIELD_E_ARG));
    DeviceGuard g(f->ps.sm.device);
    if (!g.ok) return FLDR_FIELD_E_DEVICE;
    int rc = (int)upload_input(f->ps, f->n, *frame);
    for (int k = 0; k < count && !rc; ++k) rc = enqueue_output(f, s[k], intra[k], k);
    rc = finish(f, rc, count, s, intra, host_outs, n_out, reports);
    if (!rc) f->n += 1;
    return rc;
}

extern "C" FLDR_FIELD_API int fldr_field_flush(fldr_field* f, const fldr_video_frame* host_outs, int* n_out, fldr_field_report* reports) {
    if (!f || !n_out) return FLDR_FIELD_E_ARG;
    *n_out = 0;
    if (!f->n) return 0;
    fldr_field_schedule s;
    schedule_of(f->cfg, f->j, s);
    if (s.cur > f->n - 1) return 0;                                    // every field of the frames pushed has gone out
    const bool intra = true;                                           // the last field has no successor
    CK(check_outs(f->ps, host_outs, 1, FLDR_FIELD_E_ARG));
    DeviceGuard g(f->ps.sm.device);
    if (!g.ok) return FLDR_FIELD_E_DEVICE;
    const int rc = enqueue_output(f, s, intra, 0);
    return finish(f, rc, 1, &s, &intra, host_outs, n_out, reports);
}

extern "C" FLDR_FIELD_API int fldr_field_reset(fldr_field* f) {
    if (!f) return FLDR_FIELD_E_ARG;
    forget(f);
    return 0;
}

extern "C" FLDR_FIELD_API void fldr_field_destroy(fldr_field* f) {
    if (f) { close_stream_mem(f->ps.sm); delete f; }
}
