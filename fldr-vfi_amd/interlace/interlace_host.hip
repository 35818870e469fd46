// libfldr_interlace.so, host side: validation, fldr_interlace_weave, fldr_interlace_forward (fldr_rate_forward or fldr_video_forward into
// temporaries -> one weave per field), the schedule and the stream (progressive host frames in, woven host frames out).  The video API's
// rules for formats and frames, the padded frames and the slots, pinned frames and two ends of a stream call (PaddedStream) come from
// ../video/frame_host.h; the configuration rules and the schedule of the rate converter — here run at the field rate — from
// ../rate/rate_plan.h, which includes it; the order in which several frames are checked from ../rate/tile_measure_host.h; the fill of
// a plane's walk from ../video/weave_walk_host.h.  The only fldr_* functions called are those of fldr_rate.h, fldr_video.h and
// fldr_model.h.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>

#include "../rate/rate_plan.h"
#include "../rate/tile_measure_host.h"
#include "../video/weave_walk_host.h"
#include "interlace_internal.h"

using namespace fldr_interlace_impl;

namespace {

bool filter_ok(int filter) { return (unsigned)filter <= (unsigned)FLDR_INTERLACE_COMPLEX; }

bool same_format(const fldr_video_format& a, const fldr_video_format& b) {
    return a.layout == b.layout && a.matrix == b.matrix && a.range == b.range && deep(a) == deep(b);
}

// the launch arguments of a checked call; false for a frame beyond the kernel's index arithmetic (fldr_interlace.h)
bool weave_args(int H, int W, const fldr_video_format& f, const fldr_video_frame* even, const fldr_video_frame* odd, const fldr_video_frame& out,
                WeaveArgs& a) {
    memset(&a, 0, sizeof(a));
    a.planes = planes_of(f.layout);
    a.start = even ? 0 : 1;
    a.step = even && odd ? 1 : 2;
    int64_t total = 0;
    for (int p = 0; p < a.planes; ++p) {
        WeavePlane& q = a.pl[p];
        // one work item per group and row written; the limit is that of the whole plane, whichever sources are given (fldr_interlace.h)
        if (!fill_walk(q, f, p, H, W, out, rows_of(p, H) / a.step, rows_of(p, H), total)) return false;
        bool vec = aligned16(q.out, q.pitch_out);
        if (even) { q.even = (const uint8_t*)even->plane[p]; q.pitch_even = even->pitch[p]; vec = vec && aligned16(q.even, q.pitch_even); }
        if (odd) { q.odd = (const uint8_t*)odd->plane[p]; q.pitch_odd = odd->pitch[p]; vec = vec && aligned16(q.odd, q.pitch_odd); }
        q.vec = vec ? 1 : 0;
    }
    a.total = (uint32_t)total;
    return true;
}

int check_weave(int H, int W, const fldr_video_format* fmt, const fldr_video_frame* even, const fldr_video_frame* odd, int filter,
                const fldr_video_frame* out, WeaveArgs& a) {
    if (!fmt || !out || (!even && !odd) || !size_ok(H) || W < 1 || !filter_ok(filter)) return FLDR_RATE_E_ARG;
    CK(check_format(*fmt));
    const fldr_video_frame* fr[3] = { even, odd, out };
    CK(check_frames(fr, 3, *fmt, W));
    if (!weave_args(H, W, *fmt, even, odd, *out, a)) return FLDR_RATE_E_ARG;
    for (int f = 0; f < 2; ++f) if (fr[f] && overlaps(*out, *fr[f], *fmt, H, W)) return FLDR_RATE_E_ARG;
    return 0;
}

// ---- the workspace of a forward: the rate forward's (the scene state is its last FLDR_SCENE_STATE_BYTES), then n_t temporary frames ----
struct ForwardWs { int64_t rate_bytes, fields, field_bytes, total; };

int64_t plan_ws(const fldr_model* m, int H, int W, int n_t, ForwardWs& ws) {
    if (!size_ok(H) || n_t < 1 || n_t > FLDR_RATE_MAX_OUT) return FLDR_RATE_E_ARG;
    const int64_t rb = fldr_rate_workspace_bytes(m, H, W, n_t);
    if (rb < 0) return rb;
    fldr_video_format largest;                                         // yuv420p10le: three planes of 16-bit words
    memset(&largest, 0, sizeof(largest));
    largest.layout = FLDR_VIDEO_I420; largest.depth = 10;
    ws.rate_bytes = rb;
    ws.fields = align_up(rb);
    ws.field_bytes = align_up(padded_bytes(largest, H, W));
    ws.total = ws.fields + n_t * ws.field_bytes;
    return ws.total;
}

void schedule_of(const RatePlan& p, int tff, int64_t k, fldr_interlace_schedule& s) {
    memset(&s, 0, sizeof(s));
    s.frame = k;
    s.B = p.B;
    for (int f = 0; f < 2; ++f) {
        const int64_t pos = (2 * k + f) * p.A;
        s.input[f] = pos / p.B;
        s.r[f] = pos % p.B;
        s.parity[f] = f ^ (tff ? 0 : 1);
    }
    s.push = s.input[1] + 1;
}

// the field plan of a configuration: tff, filter, reserved words (FLDR_RATE_E_ARG), then the ratio at the doubled rate (FLDR_RATE_E_RATIO)
int field_plan(const fldr_interlace_config& c, RatePlan& plan) {
    if ((unsigned)c.tff > 1u || !filter_ok(c.filter)) return FLDR_RATE_E_ARG;
    for (int i = 0; i < 4; ++i) if (c.reserved[i]) return FLDR_RATE_E_ARG;
    const fldr_rate_config& r = c.rate;
    if (r.in_num <= 0 || r.in_den <= 0 || r.out_num <= 0 || r.out_den <= 0 || r.out_num > (1 << 30)) return FLDR_RATE_E_RATIO;
    return plan_of_ratio((int64_t)r.in_num * r.out_den, 2 * (int64_t)r.in_den * r.out_num, plan);     // the doubled rate: 2^31 is no int32
}

}  // namespace

extern "C" FLDR_INTERLACE_API int fldr_interlace_version(void) { return FLDR_INTERLACE_VERSION; }

extern "C" FLDR_INTERLACE_API const char* fldr_interlace_error_string(int code) { return fldr_rate_error_string(code); }

extern "C" FLDR_INTERLACE_API int fldr_interlace_sizeof(int which) {
    switch (which) {
    case 0: return (int)sizeof(fldr_interlace_io);
    case 1: return (int)sizeof(fldr_interlace_config);
    case 2: return (int)sizeof(fldr_interlace_schedule);
    case 3: return (int)sizeof(fldr_interlace_report);
    default: return FLDR_RATE_E_ARG;
    }
}

extern "C" FLDR_INTERLACE_API int fldr_interlace_weave(int H, int W, const fldr_video_format* fmt, const fldr_video_frame* even,
                                                       const fldr_video_frame* odd, int filter, const fldr_video_frame* out, void* stream) {
    WeaveArgs a;
    CK(check_weave(H, W, fmt, even, odd, filter, out, a));
    return weave(a, luma_mode(deep(*fmt), fmt->layout), filter, (hipStream_t)stream);
}

extern "C" FLDR_INTERLACE_API int64_t fldr_interlace_workspace_bytes(const fldr_model* m, int H, int W, int n_t) {
    ForwardWs ws;
    return plan_ws(m, H, W, n_t, ws);
}

extern "C" FLDR_INTERLACE_API int fldr_interlace_field_frame(const fldr_model* m, int H, int W, const fldr_video_format* fmt, int n_t, int k, void* ws,
                                                             fldr_video_frame* frame) {
    if (!fmt || !frame || k < 0 || k >= n_t) return FLDR_RATE_E_ARG;
    ForwardWs lay;
    const int64_t total = plan_ws(m, H, W, n_t, lay);
    if (total < 0) return (int)total;
    CK(check_format(*fmt));
    if (!ws || ((uintptr_t)ws & (ALIGN - 1))) return FLDR_RATE_E_ARG;
    *frame = padded((uint8_t*)ws + lay.fields + k * lay.field_bytes, *fmt, H, W);
    return 0;
}

extern "C" FLDR_INTERLACE_API void* fldr_interlace_scene_state(const fldr_model* m, int H, int W, int n_t, void* ws) {
    ForwardWs lay;
    if (!ws || plan_ws(m, H, W, n_t, lay) < 0) return nullptr;
    return (uint8_t*)ws + lay.rate_bytes - FLDR_SCENE_STATE_BYTES;
}

extern "C" FLDR_INTERLACE_API int fldr_interlace_forward(const fldr_model* m, const fldr_interlace_io* io, void* ws, int64_t ws_bytes, void* stream) {
    if (!io) return FLDR_RATE_E_ARG;
    const fldr_video_io& v = io->pair;
    const int H = v.H, W = v.W, n_t = v.n_t;
    if (!size_ok(H) || W < 1 || n_t < 1 || n_t > FLDR_RATE_MAX_OUT || !v.t || !v.out || !io->parity || !filter_ok(io->filter) ||
        (unsigned)io->scene > 1u)
        return FLDR_RATE_E_ARG;
    for (int i = 0; i < 4; ++i) if (io->reserved[i]) return FLDR_RATE_E_ARG;
    for (int k = 0; k < n_t; ++k) if ((unsigned)io->parity[k] > 1u) return FLDR_RATE_E_ARG;
    CK(check_scene_params(io->scene_params));
    CK(check_format(v.in_format));
    CK(check_format(v.out_format));
    if (!same_format(v.in_format, v.out_format)) return FLDR_RATE_E_FORMAT;
    const fldr_video_format& fmt = v.in_format;
    const fldr_video_frame* fr[2 + FLDR_RATE_MAX_OUT] = { &v.in[0], &v.in[1] };
    for (int k = 0; k < n_t; ++k) fr[2 + k] = &v.out[k];
    CK(check_frames(fr, 2 + n_t, fmt, W));
    if (!m) return FLDR_RATE_E_ARG;
    ForwardWs lay;
    const int64_t total = plan_ws(m, H, W, n_t, lay);
    if (total < 0) return (int)total;
    if (!ws || ((uintptr_t)ws & (ALIGN - 1)) || ws_bytes < total) return FLDR_RATE_E_ARG;
    uint8_t* w = (uint8_t*)ws;
    fldr_video_frame field[FLDR_RATE_MAX_OUT];
    WeaveArgs a[FLDR_RATE_MAX_OUT];
    for (int k = 0; k < n_t; ++k) {
        field[k] = padded(w + lay.fields + k * lay.field_bytes, fmt, H, W);
        const fldr_video_frame* src = &field[k];
        if (!weave_args(H, W, fmt, io->parity[k] ? nullptr : src, io->parity[k] ? src : nullptr, v.out[k], a[k])) return FLDR_RATE_E_ARG;
        // an output anywhere inside the workspace would be written by the forward or read as a temporary
        for (int p = 0; p < planes_of(fmt.layout); ++p) {
            uintptr_t lo, hi;
            extent(v.out[k], fmt, p, H, W, lo, hi);
            if (lo < (uintptr_t)w + (uintptr_t)total && (uintptr_t)w < hi) return FLDR_RATE_E_ARG;
        }
    }
    // everything has been checked: the forward, into the temporaries, then one weave per field
    fldr_video_io vio = v;
    vio.out = field;
    if (io->scene) CK(fldr_rate_forward(m, &vio, &io->scene_params, ws, lay.rate_bytes, stream));
    else CK(fldr_video_forward(m, &vio, ws, lay.rate_bytes, stream));
    const int form = luma_mode(deep(fmt), fmt.layout);
    for (int k = 0; k < n_t; ++k) CK(weave(a[k], form, io->filter, (hipStream_t)stream));
    return 0;
}

extern "C" FLDR_INTERLACE_API int fldr_interlace_plan(const fldr_interlace_config* cfg, int64_t k, fldr_interlace_schedule* schedule) {
    if (!cfg || !schedule || k < 0 || k > (1ll << 36)) return FLDR_RATE_E_ARG;
    RatePlan plan;
    CK(field_plan(*cfg, plan));
    schedule_of(plan, cfg->tff, k, *schedule);
    return 0;
}

// ---- the stream ------------------------------------------------------------------------------------------------------------------------
constexpr int RING_MAX = FLDR_RATE_MAX_OUT / 2 + 2;

struct fldr_interlace {
    const fldr_model* model;
    fldr_interlace_config cfg;
    RatePlan plan;                     // of the FIELDS: field m at input position m A / B; max_out fields per pair
    // device, behind the slots: a ring of n_ring woven frames (frame k in k % n_ring), t, the workspace
    // pinned, behind the max_frames woven frames: t, the scene result
    PaddedStream ps;
    int64_t ws_bytes;
    int n_ring, max_frames;
    uint8_t* ring;
    float* t_dev;
    void* ws;
    float* t_host;
    fldr_scene_result* scene_host;
    fldr_interlace_report report[RING_MAX];   // of the frames in the ring, by k % n_ring
    int64_t n;                         // frames pushed since create / reset
    int64_t m;                         // the next field
};

namespace {

void forget(fldr_interlace* c) { c->n = 0; c->m = 0; }

uint8_t* ring_slot(const fldr_interlace* c, int64_t k) { return c->ring + (k % c->n_ring) * c->ps.frame_bytes; }

fldr_video_frame ring_frame(const fldr_interlace* c, int64_t k) { return padded_at(c->ps, ring_slot(c, k)); }

// field m = (i, r) enters the report of its frame; the first field of a frame begins the report
void note_field(fldr_interlace* c, int64_t m, int64_t i, int64_t r) {
    fldr_interlace_report& rep = c->report[(m >> 1) % c->n_ring];
    if (!(m & 1)) { memset(&rep, 0, sizeof(rep)); rep.frame = m >> 1; }
    rep.input[m & 1] = i;
    rep.r[m & 1] = r;
}

// the weave of field m straight from the input frame `i` (in its slot) into its frame of the ring
int enqueue_direct(fldr_interlace* c, int64_t m, int64_t i) {
    const fldr_rate_config& r = c->cfg.rate;
    const fldr_video_frame src = padded_at(c->ps, c->ps.slot[i & 1]);
    const fldr_video_frame out = ring_frame(c, m >> 1);
    const int parity = (int)(m & 1) ^ (c->cfg.tff ? 0 : 1);
    return fldr_interlace_weave(r.H, r.W, &r.format, parity ? nullptr : &src, parity ? &src : nullptr, c->cfg.filter, &out, c->ps.sm.stream);
}

// Download the frames k0 .. k0 + count - 1, one copy each, wait, hand them out with their reports; `cut`: the fields first .. first +
// n_fields - 1 with r != 0 came from the pair whose scene result is awaited here.  On a failure the object has been reset.
int finish(fldr_interlace* c, int rc, int64_t k0, int count, bool measured, int64_t first, int n_fields, const fldr_video_frame* host_outs,
           int* n_out, fldr_interlace_report* reports) {
    const uint8_t* from[RING_MAX];
    for (int q = 0; q < count; ++q) from[q] = ring_slot(c, k0 + q);
    rc = deliver(c->ps, rc, from, count, c->ps.frame_bytes, host_outs, count);
    if (rc) { forget(c); return rc; }
    if (measured && c->scene_host->cut)
        for (int64_t m = first; m < first + n_fields; ++m) {
            fldr_interlace_report& rep = c->report[(m >> 1) % c->n_ring];
            if (rep.r[m & 1]) rep.cut[m & 1] = 1;
        }
    for (int q = 0; q < count && reports; ++q) reports[q] = c->report[(k0 + q) % c->n_ring];
    *n_out = count;
    return 0;
}

}  // namespace

extern "C" FLDR_INTERLACE_API int fldr_interlace_create(const fldr_model* m, const fldr_interlace_config* cfg, fldr_interlace** out) {
    if (!cfg || !out) return FLDR_RATE_E_ARG;
    *out = nullptr;
    CK(check_rate_config(cfg->rate));
    if (!size_ok(cfg->rate.H)) return FLDR_RATE_E_ARG;
    RatePlan plan;
    CK(field_plan(*cfg, plan));
    const bool forwards = plan.B != 1;
    if (forwards && !m) return FLDR_RATE_E_ARG;
    const int H = cfg->rate.H, W = cfg->rate.W;
    const int64_t wsb = forwards ? fldr_interlace_workspace_bytes(m, H, W, plan.max_out) : 0;
    if (wsb < 0) return (int)wsb;
    if (!device_exists(cfg->rate.device)) return FLDR_RATE_E_DEVICE;
    fldr_interlace* c = new (std::nothrow) fldr_interlace();
    if (!c) return FLDR_RATE_E_DEVICE;
    c->model = m;
    c->cfg = *cfg;
    c->plan = plan;
    c->max_frames = (plan.max_out + 1) / 2;
    c->n_ring = plan.max_out / 2 + 2;                                 // the fields of one call touch at most max_out / 2 + 1 frames
    c->ws_bytes = wsb;
    const int64_t t_bytes = align_up(4ll * plan.max_out);
    if (!open_padded_stream(c->ps, cfg->rate.device, cfg->rate.format, H, W, c->n_ring, t_bytes + wsb, c->max_frames, t_bytes + ALIGN)) {
        delete c;
        return FLDR_RATE_E_DEVICE;
    }
    c->ring = c->ps.dev_rest;
    c->t_dev = (float*)(c->ring + c->n_ring * c->ps.frame_bytes);
    c->ws = forwards ? (uint8_t*)c->t_dev + t_bytes : nullptr;
    c->t_host = (float*)(c->ps.out_host + c->max_frames * c->ps.frame_bytes);
    c->scene_host = (fldr_scene_result*)((uint8_t*)c->t_host + t_bytes);
    forget(c);
    *out = c;
    return 0;
}

extern "C" FLDR_INTERLACE_API int fldr_interlace_max_out(const fldr_interlace* c) { return c ? c->max_frames : FLDR_RATE_E_ARG; }

extern "C" FLDR_INTERLACE_API int fldr_interlace_push(fldr_interlace* c, const fldr_video_frame* frame, const fldr_video_frame* host_outs, int* n_out,
                                                      fldr_interlace_report* reports) {
    if (!c || !frame || !n_out) return FLDR_RATE_E_ARG;
    *n_out = 0;
    const fldr_rate_config& r = c->cfg.rate;
    const int H = r.H, W = r.W;
    const fldr_video_format& fmt = r.format;
    CK(check_frame(*frame, fmt, W));
    // the fields of the pair (n - 1, n), by the rate converter's rule; a frame is done when its second field (an odd m) is among them
    int n_t = 0;
    int64_t r_of[FLDR_RATE_MAX_OUT];
    const int count = c->n >= 1 ? pair_outputs(c->plan, c->n, c->m, r_of, n_t) : 0;
    const int64_t k0 = c->m >> 1;                                      // the first frame this call can complete
    const int done = (int)(((c->m + count) >> 1) - k0);
    CK(check_outs(c->ps, host_outs, done, FLDR_RATE_E_ARG));
    DeviceGuard g(c->ps.sm.device);
    if (!g.ok) return FLDR_RATE_E_DEVICE;
    const hipStream_t stream = c->ps.sm.stream;
    hipError_t e;
    int rc = (int)upload_input(c->ps, c->n, *frame);
    for (int k = 0; k < count; ++k) note_field(c, c->m + k, c->n - 1, r_of[k]);
    const bool measured = n_t && r.scene == 1;
    if (!rc && n_t) {
        fill_times(r_of, count, c->plan.B, c->t_host);
        e = hipMemcpyAsync(c->t_dev, c->t_host, 4ull * n_t, hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) rc = (int)e;
        fldr_video_frame outs[FLDR_RATE_MAX_OUT];
        int32_t parity[FLDR_RATE_MAX_OUT];
        for (int k = 0, q = 0; k < count; ++k) {
            if (!r_of[k]) continue;
            outs[q] = ring_frame(c, (c->m + k) >> 1);
            parity[q++] = (int32_t)((c->m + k) & 1) ^ (c->cfg.tff ? 0 : 1);
        }
        fldr_interlace_io io;
        memset(&io, 0, sizeof(io));
        io.pair.H = H; io.pair.W = W;
        io.pair.in_format = io.pair.out_format = fmt;
        io.pair.in[0] = padded_at(c->ps, c->ps.slot[(c->n - 1) & 1]);
        io.pair.in[1] = padded_at(c->ps, c->ps.slot[c->n & 1]);
        io.pair.n_t = n_t; io.pair.t = c->t_dev; io.pair.out = outs;
        io.parity = parity;
        io.filter = c->cfg.filter;
        io.scene_params = r.scene_params;
        io.scene = r.scene;
        if (!rc) rc = fldr_interlace_forward(c->model, &io, c->ws, c->ws_bytes, stream);
        if (!rc && measured) {
            e = hipMemcpyAsync(c->scene_host, fldr_interlace_scene_state(c->model, H, W, n_t, c->ws), sizeof(fldr_scene_result),
                               hipMemcpyDeviceToHost, stream);
            if (e != hipSuccess) rc = (int)e;
        }
    }
    for (int k = 0; k < count && !rc; ++k) if (!r_of[k]) rc = enqueue_direct(c, c->m + k, c->n - 1);      // the field that lands on frame n - 1
    rc = finish(c, rc, k0, done, measured, c->m, count, host_outs, n_out, reports);
    if (rc) return rc;
    c->m += count;
    c->n += 1;
    return 0;
}

extern "C" FLDR_INTERLACE_API int fldr_interlace_flush(fldr_interlace* c, const fldr_video_frame* host_outs, int* n_out, fldr_interlace_report* reports) {
    if (!c || !n_out) return FLDR_RATE_E_ARG;
    *n_out = 0;
    if (!c->n) return 0;
    const bool due = flush_due(c->plan, c->n, c->m);                   // field m lands exactly on the last frame
    const bool held = ((c->m + (due ? 1 : 0)) & 1) != 0;               // a frame is then left with its first field only
    if (!due && !held) return 0;
    CK(check_outs(c->ps, host_outs, 1, FLDR_RATE_E_ARG));
    DeviceGuard g(c->ps.sm.device);
    if (!g.ok) return FLDR_RATE_E_DEVICE;
    int rc = 0;
    int64_t m = c->m;
    for (int f = 0; f < (due ? 1 : 0) + (held ? 1 : 0) && !rc; ++f, ++m) {
        note_field(c, m, c->n - 1, 0);
        rc = enqueue_direct(c, m, c->n - 1);
    }
    const int64_t k = (m - 1) >> 1;                                    // the last of these fields is a second field: it completes frame k
    if (held) c->report[k % c->n_ring].held = 1;
    rc = finish(c, rc, k, 1, false, 0, 0, host_outs, n_out, reports);
    if (rc) return rc;
    c->m = m;
    return 0;
}

extern "C" FLDR_INTERLACE_API int fldr_interlace_reset(fldr_interlace* c) {
    if (!c) return FLDR_RATE_E_ARG;
    forget(c);
    return 0;
}

extern "C" FLDR_INTERLACE_API void fldr_interlace_destroy(fldr_interlace* c) {
    if (c) { close_stream_mem(c->ps.sm); delete c; }
}
