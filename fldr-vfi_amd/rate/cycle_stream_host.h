// A cycle stream on the rate library, host side, written once: frames pushed one by one, every one of them measured, and of every
// `cycle` measured frames the `drop` with the smallest keys dropped and the survivors pushed into an inner fldr_rate.  Included by
// ../cadence/cadence_host.hip (the frames as they come, keyed by the repeat measure) and ../pulldown/pulldown_host.hip (the matched
// frames, keyed by the anchor rows' difference); each instantiates this text with a traits struct L that names
//   Config, Result, Report             the library's C structs: Config begins with `fldr_rate_config rate` and has cycle and drop; Report has
//                                      first_frame, n_frames, dropped_mask, moving_dropped, still_kept, cut_mask and measure[MAX_CYCLE]
//   E_ARG, E_DEVICE, MAX_CYCLE         its codes for a bad argument and a failed device or allocation, and the longest cycle it takes
//   key_less(a, b)                     the order of two results: the frame that is more of a duplicate first
//   report_frame(rep, k, res)          fills what else the report says of frame k -> whether the measure found the frame moving
// and derives its opaque stream struct S from CycleStream<L>, adding what a push uploads and measures, and forget_own(), which
// returns that part to its state after create.  What a push uploads and measures, the layout of the device and pinned blocks and
// where a cycle's first frame number comes from stay with the library.  Everything is in the unnamed namespace, like rate_plan.h.
#pragma once
#include <new>

#include "rate_plan.h"
#include "tile_measure_host.h"

namespace {

template <class L> struct CycleStream {
    typename L::Config cfg;
    fldr_rate* inner;
    int inner_max, max_out;
    StreamMem sm;
    int64_t frame_bytes;               // of a packed frame, aligned
    uint8_t* ring;                     // pinned: `cycle` packed frames, the ones the inner converter is given
    typename L::Result* result_host;   // pinned: their `cycle` results
    int64_t n;                         // frames pushed since create / reset
    int m;                             // frames of the current cycle in the ring
    bool keyed[L::MAX_CYCLE];          // ring frame k has a key (it had a previous frame)
};

template <class Config> bool cycle_ok(const Config& c, int max_cycle) {
    return c.cycle >= 1 && c.cycle <= max_cycle && c.drop >= 0 && c.drop < c.cycle;
}

// in_num (cycle - drop) / (in_den cycle), reduced; FLDR_RATE_E_RATIO when a term does not fit int32
template <class Config> int inner_rate(const Config& c, int32_t& num, int32_t& den) {
    if (c.rate.in_num <= 0 || c.rate.in_den <= 0) return FLDR_RATE_E_RATIO;
    int64_t n = (int64_t)c.rate.in_num * (c.cycle - c.drop), d = (int64_t)c.rate.in_den * c.cycle;
    reduce_terms(n, d);
    if (n > 0x7fffffffll || d > 0x7fffffffll) return FLDR_RATE_E_RATIO;
    num = (int32_t)n; den = (int32_t)d;
    return 0;
}

// fldr_*_inner_rate
template <class L> int inner_rate_entry(const typename L::Config* cfg, int32_t* num, int32_t* den) {
    if (!cfg || !num || !den || !cycle_ok(*cfg, L::MAX_CYCLE)) return L::E_ARG;
    return inner_rate(*cfg, *num, *den);
}

template <class S> void forget(S* c) {
    c->n = 0; c->m = 0;
    c->forget_own();
    (void)fldr_rate_reset(c->inner);
}

template <class S> int fail(S* c, int r) {
    drain(c->sm);
    forget(c);
    return r;
}

template <class S> uint8_t* ring_frame(const S* c, int k) { return c->ring + k * c->frame_bytes; }

// fldr_*_create.  fldr_rate_create's checks, in its order and with its codes (rate_plan.h); cycle and drop and the library's own checks
// (own_checks(config), all of them E_ARG) are judged between them and its ratio limits.  open(c) opens c->sm with the library's layout
// and points the stream's members into it -> false when that fails.
template <class L, class S, class Check, class Open>
int cycle_create(const fldr_model* m, const typename L::Config* ccfg, S** out, Check own_checks, Open open) {
    if (!ccfg || !out) return L::E_ARG;
    *out = nullptr;
    const fldr_rate_config* cfg = &ccfg->rate;
    CK(check_rate_config(*cfg));
    if (!cycle_ok(*ccfg, L::MAX_CYCLE)) return L::E_ARG;
    CK(own_checks(*ccfg));
    // the inner converter's configuration, and fldr_rate_create's limits on its ratio
    fldr_rate_config icfg = *cfg;
    CK(inner_rate(*ccfg, icfg.in_num, icfg.in_den));
    RatePlan plan;                                                     // only the limits are wanted: the inner converter makes its own
    CK(reduce_rate(icfg.in_num, icfg.in_den, icfg.out_num, icfg.out_den, plan));
    if (!m) return L::E_ARG;
    S* c = new (std::nothrow) S();
    if (!c) return L::E_DEVICE;
    c->cfg = *ccfg;
    c->inner = nullptr;
    const int rc = fldr_rate_create(m, &icfg, &c->inner);
    if (rc) { delete c; return rc; }
    c->inner_max = fldr_rate_max_out(c->inner);
    c->max_out = (ccfg->cycle - ccfg->drop) * c->inner_max + 1;
    c->frame_bytes = align_up(packed_bytes(cfg->format, cfg->H, cfg->W));
    if (!open(c)) { fldr_rate_destroy(c->inner); delete c; return L::E_DEVICE; }
    c->n = 0; c->m = 0;
    c->forget_own();
    *out = c;
    return 0;
}

// the n_drop smallest keys among the m results, the lowest frame among equals -> their mask
template <class L> uint32_t select_drops(const typename L::Result* res, const bool* keyed, int m, int n_drop) {
    uint32_t dropped = 0;
    for (int d = 0; d < n_drop; ++d) {                                 // the smallest key not yet taken
        int best = -1;
        for (int k = 0; k < m; ++k) {
            if (!keyed[k] || (dropped >> k & 1u)) continue;
            if (best < 0 || L::key_less(res[k], res[best])) best = k;
        }
        if (best < 0) break;
        dropped |= 1u << best;
    }
    return dropped;
}

// The ring holds m frames whose results have been enqueued: wait, drop n_drop of them, push the others into the inner converter.
// first_frame: the stream number of ring frame 0.  On a failure the object has been reset.
template <class L, class S>
int finish_cycle(S* c, int64_t first_frame, int n_drop, const fldr_video_frame* host_outs, int* n_out, typename L::Report* report) {
    const fldr_rate_config& rc = c->cfg.rate;
    const int m = c->m;
    const hipError_t e = hipStreamSynchronize(c->sm.stream);
    if (e != hipSuccess) { forget(c); return (int)e; }
    const uint32_t dropped = select_drops<L>(c->result_host, c->keyed, m, n_drop);
    typename L::Report rep;
    memset(&rep, 0, sizeof(rep));
    rep.first_frame = first_frame;
    rep.n_frames = (uint32_t)m;
    rep.dropped_mask = dropped;
    int total = 0, survivor = 0;
    for (int k = 0; k < m; ++k) {
        rep.measure[k] = c->result_host[k];
        const bool moving = L::report_frame(rep, k, c->result_host[k]);
        if (dropped >> k & 1u) { if (moving) ++rep.moving_dropped; continue; }
        if (c->keyed[k] && !moving) ++rep.still_kept;
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

template <class L, class S> int check_outs(const S* c, const fldr_video_frame* host_outs) {
    if (!host_outs) return L::E_ARG;
    for (int k = 0; k < c->max_out; ++k) CK(check_frame(host_outs[k], c->cfg.rate.format, c->cfg.rate.W));
    return 0;
}

// fldr_*_flush.  last(c), under the device guard, enqueues what the library still owes the ring (a failure there has been through
// fail()); then the partial cycle drops its share, and the inner converter is flushed.
template <class L, class S, class Last>
int cycle_flush(S* c, const fldr_video_frame* host_outs, int* n_out, typename L::Report* report, Last last) {
    if (!c || !n_out) return L::E_ARG;
    *n_out = 0;
    if (report) memset(report, 0, sizeof(*report));
    CK((check_outs<L>(c, host_outs)));
    DeviceGuard g(c->sm.device);
    if (!g.ok) return L::E_DEVICE;
    CK(last(c));
    int total = 0;
    if (c->m) CK((finish_cycle<L>(c, c->n - c->m, c->m * c->cfg.drop / c->cfg.cycle, host_outs, &total, report)));
    int got = 0;
    const int r = fldr_rate_flush(c->inner, host_outs + total, &got);
    if (r) { forget(c); return r; }
    *n_out = total + got;
    return 0;
}

// fldr_*_reset
template <class L, class S> int cycle_reset(S* c) {
    if (!c) return L::E_ARG;
    DeviceGuard g(c->sm.device);
    if (g.ok) drain(c->sm);
    forget(c);
    return 0;
}

// fldr_*_destroy
template <class S> void cycle_destroy(S* c) {
    if (!c) return;
    fldr_rate_destroy(c->inner);
    close_stream_mem(c->sm);
    delete c;
}

}  // namespace
