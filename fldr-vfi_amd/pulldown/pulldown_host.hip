// libfldr_pulldown.so, host side: validation, fldr_pulldown_measure, fldr_pulldown_assemble, and the pulldown stream (woven frames in,
// every frame matched to the field it belongs with, the duplicates of every cycle dropped, the survivors pushed into an inner
// fldr_rate).  The video API's rules for formats and frames, and the stream / device block / pinned block the object owns, come from
// ../video/frame_host.h; the inner converter's configuration rules come from ../rate/rate_plan.h, the checks of a luma tile measure from
// ../rate/tile_measure_host.h, and the cycle stream — the create prelude, the drop selection, the survivors' push, flush, reset — from
// ../rate/cycle_stream_host.h, which includes them all.  What is here is what a push uploads, measures and assembles and how its blocks
// are laid out.  The only fldr_* functions called are those of fldr_rate.h, fldr_video.h and fldr_model.h.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../rate/cycle_stream_host.h"
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

// H a multiple of 4 (two whole row pairs per field), and a size the tile reduce takes
bool size_ok(int H, int W) { return !(H & 3) && tiles_ok(H, W, FLDR_PULLDOWN_TILE); }

int check_measure(int H, int W, const fldr_video_format* fmt, const fldr_video_frame* cur, const fldr_video_frame* prev,
                  const fldr_video_frame* next, int anchor, const fldr_pulldown_params* p, void* state, fldr_pulldown_params& r) {
    if (!fmt || !cur || !size_ok(H, W) || (unsigned)anchor > 1u) return FLDR_RATE_E_ARG;
    CK(resolve_params(p, r));
    if (((r.allowed & P_BIT) && !prev) || ((r.allowed & N_BIT) && !next)) return FLDR_RATE_E_ARG;
    CK(check_format(*fmt));
    const fldr_video_frame* fr[3] = { cur, prev, next };
    CK(check_frames(fr, 3, *fmt, W));
    return check_state(state, FLDR_RATE_E_STATE);
}

int enqueue_measure(int H, int W, const fldr_video_format& fmt, const fldr_video_frame* cur, const fldr_video_frame* prev,
                    const fldr_video_frame* next, int anchor, const fldr_pulldown_params& r, void* state, hipStream_t s) {
    MeasureCall c;
    fill_luma(c, cur, prev, next);
    c.H = H; c.W = W; c.mode = luma_mode(deep(fmt), fmt.layout); c.anchor = anchor;
    c.comb_thresh = r.comb_thresh; c.comb_tile_min = r.comb_tile_min; c.tile_sad_min = r.tile_sad_min; c.allowed = r.allowed;
    return pulldown_measure(c, state, s);
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

// the cycle stream's view of this library (../rate/cycle_stream_host.h)
struct PulldownCycle {
    using Config = fldr_pulldown_config;
    using Result = fldr_pulldown_result;
    using Report = fldr_pulldown_report;
    static constexpr int E_ARG = FLDR_RATE_E_ARG, E_DEVICE = FLDR_RATE_E_DEVICE, MAX_CYCLE = FLDR_PULLDOWN_MAX_CYCLE;
    // (dup_max_tile_sad, dup_sad) of a before that of b
    static bool key_less(const Result& a, const Result& b) {
        return a.dup_max_tile_sad != b.dup_max_tile_sad ? a.dup_max_tile_sad < b.dup_max_tile_sad : a.dup_sad < b.dup_sad;
    }
    static bool report_frame(Report& rep, int k, const Result& res) {
        rep.match[k] = res.match;
        if (res.combed) rep.combed_mask |= 1u << k;
        return res.dup_moving_tiles != 0;
    }
};

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
struct fldr_pulldown : CycleStream<PulldownCycle> {
    fldr_pulldown_params params;       // cfg.params with the defaults filled in
    // device: three frame slots (frame i in slot i % 3), the assembled frame, the measure state.
    // pinned: cycle + 1 upload slots, the ring of `cycle` matched frames, then the `cycle` results.
    uint8_t* slot[3];
    uint8_t* out_dev;
    void* state_dev;
    uint8_t* staging;
    int64_t i;                         // frames pushed since create / reset / flush: frames i - 1, i - 2 are in their slots
    void forget_own() { i = 0; }
};

namespace {

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

}  // namespace

extern "C" FLDR_PULLDOWN_API int fldr_pulldown_inner_rate(const fldr_pulldown_config* cfg, int32_t* num, int32_t* den) {
    return inner_rate_entry<PulldownCycle>(cfg, num, den);
}

extern "C" FLDR_PULLDOWN_API int fldr_pulldown_create(const fldr_model* m, const fldr_pulldown_config* pcfg, fldr_pulldown** out) {
    fldr_pulldown_params params;
    return cycle_create<PulldownCycle>(m, pcfg, out,
        [&params](const fldr_pulldown_config& pc) {
            if (!size_ok(pc.rate.H, pc.rate.W) || (unsigned)pc.anchor > 1u || (unsigned)pc.post > 1u) return FLDR_RATE_E_ARG;
            CK(resolve_params(&pc.params, params));
            for (int i = 0; i < 4; ++i) if (pc.reserved[i]) return FLDR_RATE_E_ARG;
            return 0;
        },
        [&params](fldr_pulldown* c) {
            const int cycle = c->cfg.cycle;
            const int64_t dev_total = 4 * c->frame_bytes + FLDR_PULLDOWN_STATE_BYTES;
            const int64_t host_total = (2 * cycle + 1) * c->frame_bytes + align_up(cycle * (int64_t)sizeof(fldr_pulldown_result));
            if (!open_stream_mem(c->sm, c->cfg.rate.device, dev_total, host_total)) return false;
            c->params = params;
            for (int k = 0; k < 3; ++k) c->slot[k] = c->sm.dev + k * c->frame_bytes;
            c->out_dev = c->sm.dev + 3 * c->frame_bytes;
            c->state_dev = c->sm.dev + 4 * c->frame_bytes;
            c->staging = c->sm.pinned;
            c->ring = c->staging + (cycle + 1) * c->frame_bytes;
            c->result_host = (fldr_pulldown_result*)(c->ring + cycle * c->frame_bytes);
            return true;
        });
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
    if (completes) CK(check_outs<PulldownCycle>(c, host_outs));
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
    return completes ? finish_cycle<PulldownCycle>(c, c->n - 1 - c->cfg.cycle, c->cfg.drop, host_outs, n_out, report) : 0;
}

extern "C" FLDR_PULLDOWN_API int fldr_pulldown_flush(fldr_pulldown* c, const fldr_video_frame* host_outs, int* n_out, fldr_pulldown_report* report) {
    return cycle_flush<PulldownCycle>(c, host_outs, n_out, report, [](fldr_pulldown* c) {
        if (c->i >= 1) {                                               // the last frame: no next
            const int r = enqueue_match(c, false);
            if (r) return fail(c, r);
        }
        c->i = 0;
        return 0;
    });
}

extern "C" FLDR_PULLDOWN_API int fldr_pulldown_reset(fldr_pulldown* c) { return cycle_reset<PulldownCycle>(c); }

extern "C" FLDR_PULLDOWN_API void fldr_pulldown_destroy(fldr_pulldown* c) { cycle_destroy(c); }
