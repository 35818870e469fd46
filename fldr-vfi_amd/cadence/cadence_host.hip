// libfldr_cadence.so, host side: validation, fldr_repeat_measure, and the cadence stream (container frames in, the repeats of every
// cycle dropped, the survivors pushed into an inner fldr_rate).  The video API's rules for formats and frames, and the stream / device
// block / pinned block the object owns, come from ../video/frame_host.h; the inner converter's configuration rules come from
// ../rate/rate_plan.h, which includes it.  The only fldr_* functions called are those of fldr_rate.h, fldr_video.h and fldr_model.h.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>

#include "../rate/rate_plan.h"
#include "cadence_internal.h"

using namespace fldr_cadence_impl;

namespace {

constexpr int64_t RESULT_BYTES = sizeof(fldr_repeat_result);

// the threshold with the default filled in; FLDR_CADENCE_E_ARG outside 0 .. 261120 or with a reserved word set
int resolve_params(const fldr_repeat_params* p, int& tile_sad_min) {
    tile_sad_min = FLDR_REPEAT_TILE_SAD_DEFAULT;
    if (!p) return 0;
    if (p->tile_sad_min < 0 || p->tile_sad_min > FLDR_REPEAT_TILE_SAD_MAX) return FLDR_CADENCE_E_ARG;
    if (p->reserved[0] || p->reserved[1] || p->reserved[2]) return FLDR_CADENCE_E_ARG;
    if (p->tile_sad_min) tile_sad_min = p->tile_sad_min;
    return 0;
}

int check_measure(int H, int W, const fldr_video_format* fmt, const fldr_video_frame in[2], const fldr_repeat_params* p, void* state,
                  int& tile_sad_min) {
    const int64_t T = FLDR_REPEAT_TILE;
    if (!fmt || !in || H < 1 || W < 1 || H > 0x7fffffff - T || W > 0x7fffffff - T) return FLDR_CADENCE_E_ARG;   // rows and columns rounded up to whole tiles stay inside 32 bits
    if (((int64_t)W + T - 1) / T * (((int64_t)H + T - 1) / T) > 0x7fffffffll) return FLDR_CADENCE_E_ARG;   // the key holds the tile index in 31 bits
    int rc = resolve_params(p, tile_sad_min);
    if (!rc) rc = check_format(*fmt);
    for (int f = 0; f < 2 && !rc; ++f) rc = check_frame(in[f], *fmt, W);
    if (rc) return rc;
    if (!state || ((uintptr_t)state & (ALIGN - 1))) return FLDR_CADENCE_E_STATE;
    return 0;
}

int enqueue_measure(int H, int W, const fldr_video_format& fmt, const fldr_video_frame in[2], int tile_sad_min, void* state, hipStream_t s) {
    return repeat_measure(in[0].plane[0], in[0].pitch[0], in[1].plane[0], in[1].pitch[0], H, W, luma_mode(deep(fmt), fmt.layout), tile_sad_min,
                          state, s);
}

bool cycle_ok(const fldr_cadence_config& c) {
    return c.cycle >= 1 && c.cycle <= FLDR_CADENCE_MAX_CYCLE && c.drop >= 0 && c.drop < c.cycle;
}

// in_num (cycle - drop) / (in_den cycle), reduced; FLDR_RATE_E_RATIO when a term does not fit int32
int inner_rate(const fldr_cadence_config& c, int32_t& num, int32_t& den) {
    if (c.rate.in_num <= 0 || c.rate.in_den <= 0) return FLDR_RATE_E_RATIO;
    int64_t n = (int64_t)c.rate.in_num * (c.cycle - c.drop), d = (int64_t)c.rate.in_den * c.cycle;
    reduce_terms(n, d);
    if (n > 0x7fffffffll || d > 0x7fffffffll) return FLDR_RATE_E_RATIO;
    num = (int32_t)n; den = (int32_t)d;
    return 0;
}

// (max_tile_sad, sad) of a before that of b
bool key_less(const fldr_repeat_result& a, const fldr_repeat_result& b) {
    return a.max_tile_sad != b.max_tile_sad ? a.max_tile_sad < b.max_tile_sad : a.sad < b.sad;
}

}  // namespace

extern "C" FLDR_CADENCE_API int fldr_cadence_version(void) { return FLDR_CADENCE_VERSION; }

extern "C" FLDR_CADENCE_API const char* fldr_cadence_error_string(int code) {
    switch (code) {
    case FLDR_CADENCE_E_ARG: return "fldr_cadence: bad argument";
    case FLDR_CADENCE_E_STATE: return "fldr_cadence: repeat state missing or misaligned";
    case FLDR_CADENCE_E_DEVICE: return "fldr_cadence: no such device or out of memory";
    // above -300: the rate, video and model ranges and hipError_t, which this library passes through.  -300 .. -599 belong to the
    // shutter, light and pipe libraries, which this one never calls: such a code cannot come from here and is answered as unknown.
    default: return code > -300 ? fldr_rate_error_string(code) : "fldr_cadence: unknown error";
    }
}

extern "C" FLDR_CADENCE_API int fldr_cadence_sizeof(int which) {
    switch (which) {
    case 0: return (int)sizeof(fldr_repeat_params);
    case 1: return (int)sizeof(fldr_repeat_result);
    case 2: return (int)sizeof(fldr_cadence_config);
    case 3: return (int)sizeof(fldr_cadence_report);
    default: return FLDR_CADENCE_E_ARG;
    }
}

extern "C" FLDR_CADENCE_API int fldr_repeat_measure(int H, int W, const fldr_video_format* fmt, const fldr_video_frame in[2],
                                                    const fldr_repeat_params* p, void* state, void* stream) {
    int tile_sad_min;
    CK(check_measure(H, W, fmt, in, p, state, tile_sad_min));
    return enqueue_measure(H, W, *fmt, in, tile_sad_min, state, (hipStream_t)stream);
}

// ---- the stream ------------------------------------------------------------------------------------------------------------------------
struct fldr_cadence {
    fldr_cadence_config cfg;
    fldr_rate* inner;
    int inner_max, max_out;
    // device: slot 0, slot 1, the repeat state.  pinned: a ring of `cycle` packed frames, then `cycle` results.
    StreamMem sm;
    int64_t frame_bytes;
    uint8_t* slot[2];
    void* state_dev;
    uint8_t* ring;
    fldr_repeat_result* result_host;
    int prev;                          // slot holding the previous frame, -1 when none
    int64_t n;                         // frames pushed since create / reset
    int m;                             // frames of the current cycle in the ring
    bool keyed[FLDR_CADENCE_MAX_CYCLE];   // ring frame k has a key (it is not frame 0 of the stream)
};

namespace {

void forget(fldr_cadence* c) {
    c->prev = -1; c->n = 0; c->m = 0;
    (void)fldr_rate_reset(c->inner);
}

uint8_t* ring_frame(const fldr_cadence* c, int k) { return c->ring + k * c->frame_bytes; }

// The ring holds m frames whose measures have been enqueued: wait, drop n_drop of them, push the others into the inner converter.
// On a failure the object has been reset.
int finish_cycle(fldr_cadence* c, int n_drop, const fldr_video_frame* host_outs, int* n_out, fldr_cadence_report* report) {
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
    fldr_cadence_report rep;
    memset(&rep, 0, sizeof(rep));
    rep.first_frame = c->n - m;
    rep.n_frames = (uint32_t)m;
    rep.dropped_mask = dropped;
    int total = 0, survivor = 0;
    for (int k = 0; k < m; ++k) {
        rep.measure[k] = c->result_host[k];
        if (dropped >> k & 1u) { if (!rep.measure[k].repeat) ++rep.moving_dropped; continue; }
        if (c->keyed[k] && rep.measure[k].repeat) ++rep.still_kept;
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

int check_outs(const fldr_cadence* c, const fldr_video_frame* host_outs) {
    if (!host_outs) return FLDR_CADENCE_E_ARG;
    for (int k = 0; k < c->max_out; ++k) CK(check_frame(host_outs[k], c->cfg.rate.format, c->cfg.rate.W));
    return 0;
}

}  // namespace

extern "C" FLDR_CADENCE_API int fldr_cadence_inner_rate(const fldr_cadence_config* cfg, int32_t* num, int32_t* den) {
    if (!cfg || !num || !den || !cycle_ok(*cfg)) return FLDR_CADENCE_E_ARG;
    return inner_rate(*cfg, *num, *den);
}

extern "C" FLDR_CADENCE_API int fldr_cadence_create(const fldr_model* m, const fldr_cadence_config* ccfg, fldr_cadence** out) {
    if (!ccfg || !out) return FLDR_CADENCE_E_ARG;
    *out = nullptr;
    // fldr_rate_create's checks, in its order and with its codes (../rate/rate_plan.h); cycle and drop are judged between them and its ratio limits
    const fldr_rate_config* cfg = &ccfg->rate;
    CK(check_rate_config(*cfg));
    // this library's
    if (!cycle_ok(*ccfg)) return FLDR_CADENCE_E_ARG;
    int tile_sad_min;
    CK(resolve_params(&ccfg->repeat, tile_sad_min));
    if (ccfg->reserved[0] || ccfg->reserved[1]) return FLDR_CADENCE_E_ARG;
    // the inner converter's configuration, and fldr_rate_create's limits on its ratio
    fldr_rate_config icfg = *cfg;
    CK(inner_rate(*ccfg, icfg.in_num, icfg.in_den));
    RatePlan plan;                                                     // only the limits are wanted: the inner converter makes its own
    CK(reduce_rate(icfg.in_num, icfg.in_den, icfg.out_num, icfg.out_den, plan));
    if (!m) return FLDR_CADENCE_E_ARG;
    fldr_cadence* c = new (std::nothrow) fldr_cadence();
    if (!c) return FLDR_CADENCE_E_DEVICE;
    c->cfg = *ccfg;
    c->inner = nullptr;
    const int rc = fldr_rate_create(m, &icfg, &c->inner);
    if (rc) { delete c; return rc; }
    c->inner_max = fldr_rate_max_out(c->inner);
    c->max_out = (ccfg->cycle - ccfg->drop) * c->inner_max + 1;
    c->frame_bytes = align_up(packed_bytes(cfg->format, cfg->H, cfg->W));
    const int64_t dev_total = 2 * c->frame_bytes + FLDR_REPEAT_STATE_BYTES;
    const int64_t host_total = ccfg->cycle * c->frame_bytes + align_up(ccfg->cycle * RESULT_BYTES);
    if (!open_stream_mem(c->sm, cfg->device, dev_total, host_total)) { fldr_rate_destroy(c->inner); delete c; return FLDR_CADENCE_E_DEVICE; }
    c->slot[0] = c->sm.dev;
    c->slot[1] = c->slot[0] + c->frame_bytes;
    c->state_dev = c->slot[1] + c->frame_bytes;
    c->ring = c->sm.pinned;
    c->result_host = (fldr_repeat_result*)(c->ring + ccfg->cycle * c->frame_bytes);
    c->prev = -1; c->n = 0; c->m = 0;
    *out = c;
    return 0;
}

extern "C" FLDR_CADENCE_API int fldr_cadence_max_out(const fldr_cadence* c) { return c ? c->max_out : FLDR_CADENCE_E_ARG; }

extern "C" FLDR_CADENCE_API int fldr_cadence_push(fldr_cadence* c, const fldr_video_frame* frame, const fldr_video_frame* host_outs, int* n_out,
                                                  fldr_cadence_report* report) {
    if (!c || !frame || !n_out) return FLDR_CADENCE_E_ARG;
    *n_out = 0;
    if (report) memset(report, 0, sizeof(*report));
    const fldr_rate_config& rc = c->cfg.rate;
    const int H = rc.H, W = rc.W;
    const fldr_video_format& fmt = rc.format;
    CK(check_frame(*frame, fmt, W));
    const bool completes = c->m + 1 == c->cfg.cycle;
    if (completes) CK(check_outs(c, host_outs));
    DeviceGuard g(c->sm.device);
    if (!g.ok) return FLDR_CADENCE_E_DEVICE;
    const hipStream_t stream = c->sm.stream;
    const int k = c->m;
    const int cur = c->prev == 0 ? 1 : 0;                          // the slot not holding the previous frame
    // the ring slot was last read by the uploads and inner pushes of the cycle before, which the synchronisation of that cycle covers
    hipError_t e = upload_frame(c->sm, c->slot[cur], ring_frame(c, k), c->frame_bytes, *frame, fmt, H, W);
    int r = e == hipSuccess ? 0 : (int)e;
    c->keyed[k] = c->prev >= 0;
    if (!c->keyed[k]) memset(&c->result_host[k], 0, sizeof(fldr_repeat_result));
    if (!r && c->keyed[k]) {
        const fldr_video_frame in[2] = { packed(c->slot[c->prev], fmt, H, W), packed(c->slot[cur], fmt, H, W) };
        r = fldr_repeat_measure(H, W, &fmt, in, &c->cfg.repeat, c->state_dev, stream);
        if (!r) {
            e = hipMemcpyAsync(&c->result_host[k], c->state_dev, sizeof(fldr_repeat_result), hipMemcpyDeviceToHost, stream);
            if (e != hipSuccess) r = (int)e;
        }
    }
    if (r) { (void)hipStreamSynchronize(stream); (void)hipGetLastError(); forget(c); return r; }
    c->prev = cur;
    c->n += 1;
    c->m += 1;
    return completes ? finish_cycle(c, c->cfg.drop, host_outs, n_out, report) : 0;
}

extern "C" FLDR_CADENCE_API int fldr_cadence_flush(fldr_cadence* c, const fldr_video_frame* host_outs, int* n_out, fldr_cadence_report* report) {
    if (!c || !n_out) return FLDR_CADENCE_E_ARG;
    *n_out = 0;
    if (report) memset(report, 0, sizeof(*report));
    CK(check_outs(c, host_outs));
    DeviceGuard g(c->sm.device);
    if (!g.ok) return FLDR_CADENCE_E_DEVICE;
    int total = 0;
    if (c->m) CK(finish_cycle(c, c->m * c->cfg.drop / c->cfg.cycle, host_outs, &total, report));
    int got = 0;
    const int r = fldr_rate_flush(c->inner, host_outs + total, &got);
    if (r) { forget(c); return r; }
    *n_out = total + got;
    return 0;
}

extern "C" FLDR_CADENCE_API int fldr_cadence_reset(fldr_cadence* c) {
    if (!c) return FLDR_CADENCE_E_ARG;
    DeviceGuard g(c->sm.device);
    if (g.ok) { (void)hipStreamSynchronize(c->sm.stream); (void)hipGetLastError(); }   // nothing enqueued may still write the pinned results
    forget(c);
    return 0;
}

extern "C" FLDR_CADENCE_API void fldr_cadence_destroy(fldr_cadence* c) {
    if (!c) return;
    fldr_rate_destroy(c->inner);
    close_stream_mem(c->sm);
    delete c;
}
