// libfldr_pulldown.so, host side: validation, fldr_pulldown_measure, fldr_pulldown_assemble, and the pulldown stream (woven frames in,
// every frame matched to the field it belongs with, the duplicates of every cycle dropped, the survivors pushed into an inner
// fldr_rate).  The video API's rules for formats and frames, and the stream / device block / pinned block the object owns, come from
// ../video/frame_host.h; the inner converter's configuration rules come from ../rate/rate_plan.h, which includes it.  The only fldr_*
// functions called are those of fldr_rate.h, fldr_video.h and fldr_model.h.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>

#include "../rate/rate_plan.h"
#include "pulldown_internal.h"

using namespace fldr_pulldown_impl;

namespace {

constexpr int ALL = 7, C_BIT = 1 << FLDR_PULLDOWN_C, P_BIT = 1 << FLDR_PULLDOWN_P, N_BIT = 1 << FLDR_PULLDOWN_N;

// the parameters with the defaults filled in; FLDR_RATE_E_ARG out of range or with a reserved word set
int resolve_params(const fldr_pulldown_params* p, fldr_pulldown_params& r) {
    memset(&r, 0, sizeof(r));
    r.comb_thresh = FLDR_PULLDOWN_COMB_THRESH_DEFAULT;
    r.comb_tile_min = FLDR_PULLDOWN_COMB_TILE_DEFAULT;
    r.tile_sad_min = FLDR_PULLDOWN_TILE_SAD_DEFAULT;
    r.allowed = ALL;
    if (!p) return 0;
    if (p->comb_thresh < 0 || p->comb_thresh > 255 || p->comb_tile_min < 0 || p->comb_tile_min > FLDR_PULLDOWN_TILE_COMB_MAX ||
        p->tile_sad_min < 0 || p->tile_sad_min > FLDR_PULLDOWN_TILE_SAD_MAX || p->allowed < 0 || p->allowed > ALL)
        return FLDR_RATE_E_ARG;
    for (int i = 0; i < 4; ++i) if (p->reserved[i]) return FLDR_RATE_E_ARG;
    if (p->comb_thresh) r.comb_thresh = p->comb_thresh;
    if (p->comb_tile_min) r.comb_tile_min = p->comb_tile_min;
    if (p->tile_sad_min) r.tile_sad_min = p->tile_sad_min;
    if (p->allowed) r.allowed = p->allowed;
    return 0;
}

// H a multiple of 4, and rows and columns rounded up to whole tiles inside 32 bits with the tile index in 31
bool size_ok(int H, int W) {
    const int64_t T = FLDR_PULLDOWN_TILE;
    if (H < 4 || (H & 3) || W < 1 || H > 0x7fffffff - T || W > 0x7fffffff - T) return false;
    return ((int64_t)W + T - 1) / T * (((int64_t)H + T - 1) / T) <= 0x7fffffffll;
}

// planes, then pitches, of the frames given (null entries are skipped), in order: the video library's codes
int check_frames(const fldr_video_frame* const* fr, int n, const fldr_video_format& fmt, int W) {
    const bool words = deep(fmt);
    for (int f = 0; f < n; ++f) {
        if (!fr[f]) continue;
        for (int p = 0; p < planes_of(fmt.layout); ++p)
            if (!fr[f]->plane[p] || (words && ((uintptr_t)fr[f]->plane[p] & 1))) return FLDR_VIDEO_E_PLANE;
    }
    for (int f = 0; f < n; ++f) if (fr[f]) CK(check_frame(*fr[f], fmt, W));
    return 0;
}

int check_measure(int H, int W, const fldr_video_format* fmt, const fldr_video_frame* cur, const fldr_video_frame* prev,
                  const fldr_video_frame* next, int anchor, const fldr_pulldown_params* p, void* state, fldr_pulldown_params& r) {
    if (!fmt || !cur || !size_ok(H, W) || (unsigned)anchor > 1u) return FLDR_RATE_E_ARG;
    CK(resolve_params(p, r));
    if (((r.allowed & P_BIT) && !prev) || ((r.allowed & N_BIT) && !next)) return FLDR_RATE_E_ARG;
    CK(check_format(*fmt));
    const fldr_video_frame* fr[3] = { cur, prev, next };
    CK(check_frames(fr, 3, *fmt, W));
    if (!state || ((uintptr_t)state & (ALIGN - 1))) return FLDR_RATE_E_STATE;
    return 0;
}

int enqueue_measure(int H, int W, const fldr_video_format& fmt, const fldr_video_frame* cur, const fldr_video_frame* prev,
                    const fldr_video_frame* next, int anchor, const fldr_pulldown_params& r, void* state, hipStream_t s) {
    MeasureCall c;
    c.cur = cur->plane[0]; c.pitch_cur = cur->pitch[0];
    c.prev = prev ? prev->plane[0] : nullptr; c.pitch_prev = prev ? prev->pitch[0] : 0;
    c.next = next ? next->plane[0] : nullptr; c.pitch_next = next ? next->pitch[0] : 0;
    c.H = H; c.W = W; c.mode = luma_mode(deep(fmt), fmt.layout); c.anchor = anchor;
    c.comb_thresh = r.comb_thresh; c.comb_tile_min = r.comb_tile_min; c.tile_sad_min = r.tile_sad_min; c.allowed = r.allowed;
    return pulldown_measure(c, state, s);
}

// the bytes a plane occupies: [lo, hi)
void extent(const fldr_video_frame& f, const fldr_video_format& fmt, int p, int H, int W, uintptr_t& lo, uintptr_t& hi) {
    lo = (uintptr_t)f.plane[p];
    hi = lo + (uintptr_t)(f.pitch[p] * (rows_of(p, H) - 1) + row_bytes(fmt, p, W));
}

bool overlaps(const fldr_video_frame& out, const fldr_video_frame& in, const fldr_video_format& fmt, int H, int W) {
    for (int p = 0; p < planes_of(fmt.layout); ++p)
        for (int q = 0; q < planes_of(fmt.layout); ++q) {
            uintptr_t a0, a1, b0, b1;
            extent(out, fmt, p, H, W, a0, a1);
            extent(in, fmt, q, H, W, b0, b1);
            if (a0 < b1 && b0 < a1) return true;
        }
    return false;
}

int check_assemble(int H, int W, const fldr_video_format* fmt, const fldr_video_frame* cur, const fldr_video_frame* prev,
                   const fldr_video_frame* next, const fldr_video_frame* out, int anchor, int match, const void* decision, int post) {
    if (!fmt || !cur || !out || !size_ok(H, W) || (unsigned)anchor > 1u || match < -1 || match > 2 || (unsigned)post > 1u) return FLDR_RATE_E_ARG;
    if (match < 0 && (!decision || ((uintptr_t)decision & 3))) return FLDR_RATE_E_ARG;
    if ((match == FLDR_PULLDOWN_P && !prev) || (match == FLDR_PULLDOWN_N && !next)) return FLDR_RATE_E_ARG;
    CK(check_format(*fmt));
    const fldr_video_frame* fr[4] = { cur, prev, next, out };
    CK(check_frames(fr, 4, *fmt, W));
    for (int f = 0; f < 3; ++f) if (fr[f] && overlaps(*out, *fr[f], *fmt, H, W)) return FLDR_RATE_E_ARG;
    return 0;
}

int enqueue_assemble(int H, int W, const fldr_video_format& fmt, const fldr_video_frame* cur, const fldr_video_frame* prev,
                     const fldr_video_frame* next, const fldr_video_frame* out, int anchor, int match, int combed, const void* decision,
                     int post, hipStream_t s) {
    AssembleCall c;
    if (!prev) prev = cur;                                             // a missing frame stands for cur: it is never chosen
    if (!next) next = cur;
    c.n_planes = planes_of(fmt.layout);
    for (int p = 0; p < c.n_planes; ++p) {
        AssemblePlane& a = c.plane[p];
        a.cur = (const uint8_t*)cur->plane[p]; a.prev = (const uint8_t*)prev->plane[p]; a.next = (const uint8_t*)next->plane[p];
        a.out = (uint8_t*)out->plane[p];
        a.pitch_cur = cur->pitch[p]; a.pitch_prev = prev->pitch[p]; a.pitch_next = next->pitch[p]; a.pitch_out = out->pitch[p];
        a.row_bytes = row_bytes(fmt, p, W);
        a.rows = rows_of(p, H);
        a.vec = luma_vec_ok(a.cur, a.pitch_cur, a.prev, a.pitch_prev) && luma_vec_ok(a.next, a.pitch_next, a.out, a.pitch_out);
    }
    c.mode = luma_mode(deep(fmt), fmt.layout);
    c.anchor = anchor; c.match = match; c.combed = combed; c.decision = (const int32_t*)decision; c.post = post;
    return pulldown_assemble(c, s);
}

bool cycle_ok(const fldr_pulldown_config& c) {
    return c.cycle >= 1 && c.cycle <= FLDR_PULLDOWN_MAX_CYCLE && c.drop >= 0 && c.drop < c.cycle;
}

// in_num (cycle - drop) / (in_den cycle), reduced; FLDR_RATE_E_RATIO when a term does not fit int32
int inner_rate(const fldr_pulldown_config& c, int32_t& num, int32_t& den) {
    if (c.rate.in_num <= 0 || c.rate.in_den <= 0) return FLDR_RATE_E_RATIO;
    int64_t n = (int64_t)c.rate.in_num * (c.cycle - c.drop), d = (int64_t)c.rate.in_den * c.cycle;
    reduce_terms(n, d);
    if (n > 0x7fffffffll || d > 0x7fffffffll) return FLDR_RATE_E_RATIO;
    num = (int32_t)n; den = (int32_t)d;
    return 0;
}

// (dup_max_tile_sad, dup_sad) of a before that of b
bool key_less(const fldr_pulldown_result& a, const fldr_pulldown_result& b) {
    return a.dup_max_tile_sad != b.dup_max_tile_sad ? a.dup_max_tile_sad < b.dup_max_tile_sad : a.dup_sad < b.dup_sad;
}

}  // namespace

extern "C" FLDR_PULLDOWN_API int fldr_pulldown_version(void) { return FLDR_PULLDOWN_VERSION; }

extern "C" FLDR_PULLDOWN_API const char* fldr_pulldown_error_string(int code) { return fldr_rate_error_string(code); }

extern "C" FLDR_PULLDOWN_API int fldr_pulldown_sizeof(int which) {
    switch (which) {
    case 0: return (int)sizeof(fldr_pulldown_params);
    case 1: return (int)sizeof(fldr_pulldown_result);
    case 2: return (int)sizeof(fldr_pulldown_config);
    case 3: return (int)sizeof(fldr_pulldown_report);
    default: return FLDR_RATE_E_ARG;
    }
}

extern "C" FLDR_PULLDOWN_API int fldr_pulldown_measure(int H, int W, const fldr_video_format* fmt, const fldr_video_frame* cur,
                                                       const fldr_video_frame* prev, const fldr_video_frame* next, int anchor,
                                                       const fldr_pulldown_params* p, void* state, void* stream) {
    fldr_pulldown_params r;
    CK(check_measure(H, W, fmt, cur, prev, next, anchor, p, state, r));
    return enqueue_measure(H, W, *fmt, cur, prev, next, anchor, r, state, (hipStream_t)stream);
}

extern "C" FLDR_PULLDOWN_API int fldr_pulldown_assemble(int H, int W, const fldr_video_format* fmt, const fldr_video_frame* cur,
                                                        const fldr_video_frame* prev, const fldr_video_frame* next,
                                                        const fldr_video_frame* out, int anchor, int match, int combed, const void* decision,
                                                        int post, void* stream) {
    CK(check_assemble(H, W, fmt, cur, prev, next, out, anchor, match, decision, post));
    return enqueue_assemble(H, W, *fmt, cur, prev, next, out, anchor, match, combed, decision, post, (hipStream_t)stream);
}

// ---- the stream ------------------------------------------------------------------------------------------------------------------------
struct fldr_pulldown {
    fldr_pulldown_config cfg;
    fldr_pulldown_params params;       // cfg.params with the defaults filled in
    fldr_rate* inner;
    int inner_max, max_out;
    // device: three frame slots (frame i in slot i % 3), the assembled frame, the measure state.
    // pinned: cycle + 1 upload slots, a ring of `cycle` matched frames, then `cycle` results.
    StreamMem sm;
    int64_t frame_bytes;
    uint8_t* slot[3];
    uint8_t* out_dev;
    void* state_dev;
    uint8_t* staging;
    uint8_t* ring;
    fldr_pulldown_result* result_host;
    int64_t n;                         // frames pushed since create / reset
    int64_t i;                         // frames pushed since create / reset / flush: frames i - 1, i - 2 are in their slots
    int m;                             // matched frames of the current cycle in the ring
    bool keyed[FLDR_PULLDOWN_MAX_CYCLE];   // ring frame k has a key (it had a previous frame)
};

namespace {

void forget(fldr_pulldown* c) {
    c->n = 0; c->i = 0; c->m = 0;
    (void)fldr_rate_reset(c->inner);
}

uint8_t* ring_frame(const fldr_pulldown* c, int k) { return c->ring + k * c->frame_bytes; }

// Enqueue measure, assemble and the two downloads of frame i - 1 (prev: frame i - 2 when there is one; next: frame i when has_next).
int enqueue_match(fldr_pulldown* c, bool has_next) {
    const fldr_rate_config& rc = c->cfg.rate;
    const int H = rc.H, W = rc.W;
    const fldr_video_format& fmt = rc.format;
    const hipStream_t stream = c->sm.stream;
    const bool has_prev = c->i >= 2;
    const fldr_video_frame cur = packed(c->slot[(c->i - 1) % 3], fmt, H, W);
    const fldr_video_frame prev = packed(c->slot[(c->i + 1) % 3], fmt, H, W);      // (i - 2) % 3
    const fldr_video_frame next = packed(c->slot[c->i % 3], fmt, H, W);
    fldr_pulldown_params p = c->params;
    p.allowed &= C_BIT | (has_prev ? P_BIT : 0) | (has_next ? N_BIT : 0);
    if (!p.allowed) p.allowed = C_BIT;
    const int k = c->m;
    CK(fldr_pulldown_measure(H, W, &fmt, &cur, has_prev ? &prev : nullptr, has_next ? &next : nullptr, c->cfg.anchor, &p, c->state_dev, stream));
    const fldr_video_frame out = packed(c->out_dev, fmt, H, W);
    CK(fldr_pulldown_assemble(H, W, &fmt, &cur, has_prev ? &prev : nullptr, has_next ? &next : nullptr, &out, c->cfg.anchor, -1, 0,
                              c->state_dev, c->cfg.post, stream));
    hipError_t e = hipMemcpyAsync(ring_frame(c, k), c->out_dev, (size_t)c->frame_bytes, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&c->result_host[k], c->state_dev, sizeof(fldr_pulldown_result), hipMemcpyDeviceToHost, stream);
    if (e != hipSuccess) return (int)e;
    c->keyed[k] = has_prev;
    c->m += 1;
    return 0;
}

// The ring holds m matched frames whose downloads have been enqueued: wait, drop n_drop of them, push the others into the inner
// converter.  On a failure the object has been reset.
int finish_cycle(fldr_pulldown* c, int64_t first_frame, int n_drop, const fldr_video_frame* host_outs, int* n_out, fldr_pulldown_report* report) {
    const fldr_rate_config& rc = c->cfg.rate;
    const int m = c->m;
    const hipError_t e = hipStreamSynchronize(c->sm.stream);
    if (e != hipSuccess) { forget(c); return (int)e; }
    uint32_t dropped = 0;
    for (int d = 0; d < n_drop; ++d) {                                 // the smallest key not yet taken, the lowest frame among equals
        int best = -1;
        for (int k = 0; k < m; ++k) {
            if (!c->keyed[k] || (dropped >> k & 1u)) continue;
            if (best < 0 || key_less(c->result_host[k], c->result_host[best])) best = k;
        }
        if (best < 0) break;
        dropped |= 1u << best;
    }
    fldr_pulldown_report rep;
    memset(&rep, 0, sizeof(rep));
    rep.first_frame = first_frame;
    rep.n_frames = (uint32_t)m;
    rep.dropped_mask = dropped;
    int total = 0, survivor = 0;
    for (int k = 0; k < m; ++k) {
        const fldr_pulldown_result& res = c->result_host[k];
        rep.measure[k] = res;
        rep.match[k] = res.match;
        if (res.combed) rep.combed_mask |= 1u << k;
        if (dropped >> k & 1u) { if (res.dup_moving_tiles) ++rep.moving_dropped; continue; }
        if (c->keyed[k] && !res.dup_moving_tiles) ++rep.still_kept;
        const fldr_video_frame fr = packed(ring_frame(c, k), rc.format, rc.H, rc.W);
        fldr_scene_result scene;
        int got = 0;
        const int r = fldr_rate_push(c->inner, &fr, host_outs + total, &got, &scene);
        if (r) { forget(c); *n_out = 0; return r; }
        if (scene.cut) rep.cut_mask |= 1u << survivor;
        total += got;
        ++survivor;
    }
    c->m = 0;
    *n_out = total;
    if (report) *report = rep;
    return 0;
}

int check_outs(const fldr_pulldown* c, const fldr_video_frame* host_outs) {
    if (!host_outs) return FLDR_RATE_E_ARG;
    for (int k = 0; k < c->max_out; ++k) CK(check_frame(host_outs[k], c->cfg.rate.format, c->cfg.rate.W));
    return 0;
}

int fail(fldr_pulldown* c, int r) {
    (void)hipStreamSynchronize(c->sm.stream);
    (void)hipGetLastError();
    forget(c);
    return r;
}

}  // namespace

extern "C" FLDR_PULLDOWN_API int fldr_pulldown_inner_rate(const fldr_pulldown_config* cfg, int32_t* num, int32_t* den) {
    if (!cfg || !num || !den || !cycle_ok(*cfg)) return FLDR_RATE_E_ARG;
    return inner_rate(*cfg, *num, *den);
}

extern "C" FLDR_PULLDOWN_API int fldr_pulldown_create(const fldr_model* m, const fldr_pulldown_config* pcfg, fldr_pulldown** out) {
    if (!pcfg || !out) return FLDR_RATE_E_ARG;
    *out = nullptr;
    // fldr_rate_create's checks, in its order and with its codes (../rate/rate_plan.h); this library's are judged between them and its ratio limits
    const fldr_rate_config* cfg = &pcfg->rate;
    CK(check_rate_config(*cfg));
    if (!size_ok(cfg->H, cfg->W) || !cycle_ok(*pcfg) || (unsigned)pcfg->anchor > 1u || (unsigned)pcfg->post > 1u) return FLDR_RATE_E_ARG;
    fldr_pulldown_params params;
    CK(resolve_params(&pcfg->params, params));
    for (int i = 0; i < 4; ++i) if (pcfg->reserved[i]) return FLDR_RATE_E_ARG;
    // the inner converter's configuration, and fldr_rate_create's limits on its ratio
    fldr_rate_config icfg = *cfg;
    CK(inner_rate(*pcfg, icfg.in_num, icfg.in_den));
    RatePlan plan;                                                     // only the limits are wanted: the inner converter makes its own
    CK(reduce_rate(icfg.in_num, icfg.in_den, icfg.out_num, icfg.out_den, plan));
    if (!m) return FLDR_RATE_E_ARG;
    fldr_pulldown* c = new (std::nothrow) fldr_pulldown();
    if (!c) return FLDR_RATE_E_DEVICE;
    c->cfg = *pcfg;
    c->params = params;
    c->inner = nullptr;
    const int rc = fldr_rate_create(m, &icfg, &c->inner);
    if (rc) { delete c; return rc; }
    c->inner_max = fldr_rate_max_out(c->inner);
    c->max_out = (pcfg->cycle - pcfg->drop) * c->inner_max + 1;
    c->frame_bytes = align_up(packed_bytes(cfg->format, cfg->H, cfg->W));
    const int64_t dev_total = 4 * c->frame_bytes + FLDR_PULLDOWN_STATE_BYTES;
    const int64_t host_total = (2 * pcfg->cycle + 1) * c->frame_bytes + align_up(pcfg->cycle * (int64_t)sizeof(fldr_pulldown_result));
    if (!open_stream_mem(c->sm, cfg->device, dev_total, host_total)) { fldr_rate_destroy(c->inner); delete c; return FLDR_RATE_E_DEVICE; }
    for (int k = 0; k < 3; ++k) c->slot[k] = c->sm.dev + k * c->frame_bytes;
    c->out_dev = c->sm.dev + 3 * c->frame_bytes;
    c->state_dev = c->sm.dev + 4 * c->frame_bytes;
    c->staging = c->sm.pinned;
    c->ring = c->staging + (pcfg->cycle + 1) * c->frame_bytes;
    c->result_host = (fldr_pulldown_result*)(c->ring + pcfg->cycle * c->frame_bytes);
    c->n = 0; c->i = 0; c->m = 0;
    *out = c;
    return 0;
}

extern "C" FLDR_PULLDOWN_API int fldr_pulldown_max_out(const fldr_pulldown* c) { return c ? c->max_out : FLDR_RATE_E_ARG; }

extern "C" FLDR_PULLDOWN_API int fldr_pulldown_push(fldr_pulldown* c, const fldr_video_frame* frame, const fldr_video_frame* host_outs, int* n_out,
                                                    fldr_pulldown_report* report) {
    if (!c || !frame || !n_out) return FLDR_RATE_E_ARG;
    *n_out = 0;
    if (report) memset(report, 0, sizeof(*report));
    const fldr_rate_config& rc = c->cfg.rate;
    CK(check_frame(*frame, rc.format, rc.W));
    const bool completes = c->i >= 1 && c->m + 1 == c->cfg.cycle;    // this push matches frame i - 1, the cycle's last
    if (completes) CK(check_outs(c, host_outs));
    DeviceGuard g(c->sm.device);
    if (!g.ok) return FLDR_RATE_E_DEVICE;
    // An upload slot is written again cycle + 1 pushes later.  Any cycle + 1 pushes in a row hold one that completed a cycle, and so
    // synchronised after enqueueing its own upload: the copy out of this slot has been waited for.
    uint8_t* up = c->staging + (c->i % (c->cfg.cycle + 1)) * c->frame_bytes;
    const hipError_t e = upload_frame(c->sm, c->slot[c->i % 3], up, c->frame_bytes, *frame, rc.format, rc.H, rc.W);
    if (e != hipSuccess) return fail(c, (int)e);
    if (c->i >= 1) {
        const int r = enqueue_match(c, true);
        if (r) return fail(c, r);
    }
    c->i += 1;
    c->n += 1;
    // the cycle's frames are n - 1 - cycle .. n - 2: the frame just pushed is not matched yet
    return completes ? finish_cycle(c, c->n - 1 - c->cfg.cycle, c->cfg.drop, host_outs, n_out, report) : 0;
}

extern "C" FLDR_PULLDOWN_API int fldr_pulldown_flush(fldr_pulldown* c, const fldr_video_frame* host_outs, int* n_out, fldr_pulldown_report* report) {
    if (!c || !n_out) return FLDR_RATE_E_ARG;
    *n_out = 0;
    if (report) memset(report, 0, sizeof(*report));
    CK(check_outs(c, host_outs));
    DeviceGuard g(c->sm.device);
    if (!g.ok) return FLDR_RATE_E_DEVICE;
    int total = 0;
    if (c->i >= 1) {                                                   // the last frame: no next
        const int r = enqueue_match(c, false);
        if (r) return fail(c, r);
        const int m = c->m;
        CK(finish_cycle(c, c->n - m, m * c->cfg.drop / c->cfg.cycle, host_outs, &total, report));
    }
    c->i = 0;
    int got = 0;
    const int r = fldr_rate_flush(c->inner, host_outs + total, &got);
    if (r) { forget(c); return r; }
    *n_out = total + got;
    return 0;
}

extern "C" FLDR_PULLDOWN_API int fldr_pulldown_reset(fldr_pulldown* c) {
    if (!c) return FLDR_RATE_E_ARG;
    DeviceGuard g(c->sm.device);
    if (g.ok) { (void)hipStreamSynchronize(c->sm.stream); (void)hipGetLastError(); }   // nothing enqueued may still write the pinned ring
    forget(c);
    return 0;
}

extern "C" FLDR_PULLDOWN_API void fldr_pulldown_destroy(fldr_pulldown* c) {
    if (!c) return;
    fldr_rate_destroy(c->inner);
    close_stream_mem(c->sm);
    delete c;
}
