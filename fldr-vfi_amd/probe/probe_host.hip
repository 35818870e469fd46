// libfldr_probe.so, host side: validation, fldr_probe_measure, the classifier (fldr_probe_frame_class, fldr_probe_classify: pure host
// functions) and the probe stream (host frames in, three of them on the device, every frame but the first measured against its two
// neighbours, the results in a pinned ring, a verdict on demand).  The video API's rules for formats and frames, and the stream / device
// block / pinned block the object owns, come from ../video/frame_host.h; the checks a luma tile measure shares with the cadence and
// pulldown libraries' come from ../rate/tile_measure_host.h, which includes it.  The only fldr_* function called is fldr_rate_error_string.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>

#include "../rate/tile_measure_host.h"
#include "probe_internal.h"

using namespace fldr_probe_impl;

namespace {

// the parameters with the defaults filled in; FLDR_RATE_E_ARG out of range or with a reserved word set
int resolve_params(const fldr_probe_params* p, fldr_probe_params& r) {
    memset(&r, 0, sizeof(r));
    r.comb_thresh = FLDR_PROBE_COMB_THRESH_DEFAULT;
    r.comb_tile_min = FLDR_PROBE_COMB_TILE_DEFAULT;
    r.tile_sad_min = FLDR_PROBE_TILE_SAD_DEFAULT;
    r.frame_tile_sad_min = FLDR_PROBE_FRAME_TILE_SAD_DEFAULT;
    r.min_moved = FLDR_PROBE_MIN_MOVED_DEFAULT;
    if (!p) return 0;
    if (p->comb_thresh < 0 || p->comb_thresh > 255 || p->comb_tile_min < 0 || p->comb_tile_min > FLDR_PROBE_TILE_COMB_MAX ||
        p->tile_sad_min < 0 || p->tile_sad_min > FLDR_PROBE_TILE_SAD_MAX || p->frame_tile_sad_min < 0 ||
        p->frame_tile_sad_min > FLDR_PROBE_FRAME_TILE_SAD_MAX || p->min_moved < 0 || p->min_moved > 64 || p->max_outliers < 0 ||
        p->max_outliers > 64 || (unsigned)p->anchor > 1u)
        return FLDR_RATE_E_ARG;
    for (int i = 0; i < 5; ++i) if (p->reserved[i]) return FLDR_RATE_E_ARG;
    if (p->comb_thresh) r.comb_thresh = p->comb_thresh;
    if (p->comb_tile_min) r.comb_tile_min = p->comb_tile_min;
    if (p->tile_sad_min) r.tile_sad_min = p->tile_sad_min;
    if (p->frame_tile_sad_min) r.frame_tile_sad_min = p->frame_tile_sad_min;
    if (p->min_moved) r.min_moved = p->min_moved;
    r.max_outliers = p->max_outliers;
    r.anchor = p->anchor;
    return 0;
}

// H a multiple of 4 (two whole row pairs per field), and a size the tile reduce takes
bool size_ok(int H, int W) { return !(H & 3) && tiles_ok(H, W, FLDR_PROBE_TILE); }

int check_measure(int H, int W, const fldr_video_format* fmt, const fldr_video_frame* cur, const fldr_video_frame* prev,
                  const fldr_video_frame* next, const fldr_probe_params* p, void* state, fldr_probe_params& r) {
    if (!fmt || !cur || !size_ok(H, W)) return FLDR_RATE_E_ARG;
    CK(resolve_params(p, r));
    CK(check_format(*fmt));
    const fldr_video_frame* fr[3] = { cur, prev, next };
    CK(check_frames(fr, 3, *fmt, W));
    return check_state(state, FLDR_RATE_E_STATE);
}

int enqueue_measure(int H, int W, const fldr_video_format& fmt, const fldr_video_frame* cur, const fldr_video_frame* prev,
                    const fldr_video_frame* next, const fldr_probe_params& r, void* state, hipStream_t s) {
    MeasureCall c;
    fill_luma(c, cur, prev, next);
    c.H = H; c.W = W; c.mode = luma_mode(deep(fmt), fmt.layout);
    c.comb_thresh = r.comb_thresh; c.tile_sad_min = r.tile_sad_min; c.frame_tile_sad_min = r.frame_tile_sad_min;
    return probe_measure(c, state, s);
}

// ---- the classifier ----------------------------------------------------------------------------------------------------------------------
int frame_class(const fldr_probe_result& r, const fldr_probe_params& p) {
    if (r.frame_moving_tiles == 0) return FLDR_PROBE_FRAME_STILL;
    const uint32_t min_comb = (uint32_t)p.comb_tile_min;
    if (r.max_tile_comb[0][FLDR_PROBE_C] < min_comb && r.max_tile_comb[1][FLDR_PROBE_C] < min_comb) return FLDR_PROBE_FRAME_PROG;
    bool film = true;
    for (int q = 0; q < 2; ++q) {
        uint32_t best = r.max_tile_comb[q][0];
        for (int k = 1; k < 3; ++k) if (r.max_tile_comb[q][k] < best) best = r.max_tile_comb[q][k];
        if (best >= min_comb) film = false;
    }
    return film ? FLDR_PROBE_FRAME_FILM : FLDR_PROBE_FRAME_VIDEO;
}

void classify(const fldr_probe_result* rs, int M, const fldr_probe_params& p, fldr_probe_verdict& v) {
    memset(&v, 0, sizeof(v));
    v.kind = FLDR_PROBE_UNKNOWN; v.tff = -1; v.cycle = 1; v.anchor = p.anchor; v.n_frames = M;
    for (int n = 0; n < M; ++n) {
        switch (frame_class(rs[n], p)) {
        case FLDR_PROBE_FRAME_STILL: ++v.n_still; break;
        case FLDR_PROBE_FRAME_PROG: ++v.n_prog; break;
        case FLDR_PROBE_FRAME_FILM: ++v.n_film; break;
        default:
            ++v.n_video;
            if (rs[n].tff_sum < rs[n].bff_sum) ++v.votes_tff;
            else if (rs[n].tff_sum > rs[n].bff_sum) ++v.votes_bff;
        }
    }
    v.n_moved = v.n_prog + v.n_film + v.n_video;
    if (v.n_moved < p.min_moved) return;
    const int n_prog = v.n_prog > p.max_outliers ? v.n_prog : 0, n_film = v.n_film > p.max_outliers ? v.n_film : 0,
              n_video = v.n_video > p.max_outliers ? v.n_video : 0;
    if (!n_video && !n_film) v.kind = FLDR_PROBE_PROGRESSIVE;
    else if (!n_video) v.kind = FLDR_PROBE_FILM;
    else if (!n_film) {
        v.kind = FLDR_PROBE_INTERLACED;
        v.tff = v.votes_tff > v.votes_bff ? 1 : v.votes_tff < v.votes_bff ? 0 : -1;
        v.mixed = n_prog > 0;
    } else v.kind = FLDR_PROBE_MIXED;
    if (v.kind != FLDR_PROBE_PROGRESSIVE && v.kind != FLDR_PROBE_FILM) return;
    const bool film = v.kind == FLDR_PROBE_FILM;
    auto r = [&](int n) { return film ? rs[n].field_moving_tiles[p.anchor] == 0 : rs[n].frame_moving_tiles == 0; };
    bool any = false;
    for (int n = 0; n < M; ++n) any = any || r(n);
    if (!any) return;                                                  // 1, 0
    int cycle = 0;
    for (int c = 1; c <= FLDR_PROBE_MAX_CYCLE && c < M && !cycle; ++c) {
        bool ok = true;
        for (int n = 0; n + c < M && ok; ++n) ok = r(n) == r(n + c);
        if (ok) cycle = c;
    }
    if (!cycle) { v.irregular = 1; return; }
    v.cycle = cycle;
    for (int n = 0; n < cycle; ++n) v.drop += r(n) ? 1 : 0;
    for (int n = 0; n + cycle < M; ++n) v.confirmed += r(n) && r(n + cycle) ? 1 : 0;
}

}  // namespace

extern "C" FLDR_PROBE_API int fldr_probe_version(void) { return FLDR_PROBE_VERSION; }

extern "C" FLDR_PROBE_API const char* fldr_probe_error_string(int code) { return fldr_rate_error_string(code); }

extern "C" FLDR_PROBE_API int fldr_probe_sizeof(int which) {
    switch (which) {
    case 0: return (int)sizeof(fldr_probe_params);
    case 1: return (int)sizeof(fldr_probe_result);
    case 2: return (int)sizeof(fldr_probe_verdict);
    case 3: return (int)sizeof(fldr_probe_config);
    default: return FLDR_RATE_E_ARG;
    }
}

extern "C" FLDR_PROBE_API int fldr_probe_measure(int H, int W, const fldr_video_format* fmt, const fldr_video_frame* cur,
                                                 const fldr_video_frame* prev, const fldr_video_frame* next, const fldr_probe_params* p,
                                                 void* state, void* stream) {
    fldr_probe_params r;
    CK(check_measure(H, W, fmt, cur, prev, next, p, state, r));
    return enqueue_measure(H, W, *fmt, cur, prev, next, r, state, (hipStream_t)stream);
}

extern "C" FLDR_PROBE_API int fldr_probe_frame_class(const fldr_probe_result* r, const fldr_probe_params* p) {
    fldr_probe_params q;
    if (!r) return FLDR_RATE_E_ARG;
    CK(resolve_params(p, q));
    return frame_class(*r, q);
}

extern "C" FLDR_PROBE_API int fldr_probe_classify(const fldr_probe_result* results, int M, const fldr_probe_params* p, fldr_probe_verdict* out) {
    fldr_probe_params q;
    if (!out || M < 0 || (M > 0 && !results)) return FLDR_RATE_E_ARG;
    CK(resolve_params(p, q));
    classify(results, M, q, *out);
    return 0;
}

// ---- the stream ------------------------------------------------------------------------------------------------------------------------
struct fldr_probe {
    fldr_probe_config cfg;
    fldr_probe_params params;          // cfg.params with the defaults filled in
    // device: three frame slots (frame i in slot i % 3), the measure state.
    // pinned: three upload slots (frame i through slot i % 3), then the ring of `window` results.
    StreamMem sm;
    int64_t frame_bytes;
    uint8_t* slot[3];
    void* state_dev;
    uint8_t* staging[3];
    hipEvent_t uploaded[3];            // recorded behind the copy out of each upload slot
    fldr_probe_result* ring;
    int64_t n;                         // frames pushed since create / reset
    int64_t measured;                  // results enqueued since create / reset: of frames 1 .. measured, result j in ring[(j - 1) % window]
};

namespace {

void forget(fldr_probe* c) { c->n = 0; c->measured = 0; }

int fail(fldr_probe* c, int r) {
    drain(c->sm);
    forget(c);
    return r;
}

// wait for everything enqueued; on a failure the object has been reset
int settle(fldr_probe* c) {
    DeviceGuard g(c->sm.device);
    if (!g.ok) return FLDR_RATE_E_DEVICE;
    const hipError_t e = hipStreamSynchronize(c->sm.stream);
    if (e != hipSuccess) { (void)hipGetLastError(); forget(c); return (int)e; }
    return 0;
}

int held(const fldr_probe* c) { return (int)(c->measured < c->cfg.window ? c->measured : c->cfg.window); }

void destroy(fldr_probe* c) {
    {
        DeviceGuard g(c->sm.device);
        for (int k = 0; k < 3; ++k) if (c->uploaded[k]) (void)hipEventDestroy(c->uploaded[k]);
    }
    close_stream_mem(c->sm);
    delete c;
}

}  // namespace

extern "C" FLDR_PROBE_API int fldr_probe_create(const fldr_probe_config* cfg, fldr_probe** out) {
    if (!cfg || !out) return FLDR_RATE_E_ARG;
    *out = nullptr;
    if (!size_ok(cfg->H, cfg->W) || cfg->device < 0 || cfg->window < FLDR_PROBE_MIN_WINDOW || cfg->window > FLDR_PROBE_MAX_WINDOW)
        return FLDR_RATE_E_ARG;
    fldr_probe_params params;
    CK(resolve_params(&cfg->params, params));
    for (int i = 0; i < 4; ++i) if (cfg->reserved[i]) return FLDR_RATE_E_ARG;
    CK(check_format(cfg->format));
    fldr_probe* c = new (std::nothrow) fldr_probe();
    if (!c) return FLDR_RATE_E_DEVICE;
    c->cfg = *cfg;
    c->params = params;
    for (int k = 0; k < 3; ++k) c->uploaded[k] = nullptr;
    c->frame_bytes = align_up(packed_bytes(cfg->format, cfg->H, cfg->W));
    const int64_t dev_total = 3 * c->frame_bytes + FLDR_PROBE_STATE_BYTES;
    const int64_t host_total = 3 * c->frame_bytes + align_up(cfg->window * (int64_t)sizeof(fldr_probe_result));
    if (!open_stream_mem(c->sm, cfg->device, dev_total, host_total)) { delete c; return FLDR_RATE_E_DEVICE; }
    {
        DeviceGuard g(cfg->device);
        for (int k = 0; k < 3; ++k)
            if (!g.ok || hipEventCreateWithFlags(&c->uploaded[k], hipEventDisableTiming) != hipSuccess) {
                c->uploaded[k] = nullptr;
                (void)hipGetLastError();
                destroy(c);
                return FLDR_RATE_E_DEVICE;
            }
    }
    for (int k = 0; k < 3; ++k) {
        c->slot[k] = c->sm.dev + k * c->frame_bytes;
        c->staging[k] = c->sm.pinned + k * c->frame_bytes;
    }
    c->state_dev = c->sm.dev + 3 * c->frame_bytes;
    c->ring = (fldr_probe_result*)(c->sm.pinned + 3 * c->frame_bytes);
    forget(c);
    *out = c;
    return 0;
}

extern "C" FLDR_PROBE_API int fldr_probe_push(fldr_probe* c, const fldr_video_frame* frame) {
    if (!c || !frame) return FLDR_RATE_E_ARG;
    const fldr_probe_config& cf = c->cfg;
    CK(check_frame(*frame, cf.format, cf.W));
    DeviceGuard g(c->sm.device);
    if (!g.ok) return FLDR_RATE_E_DEVICE;
    const hipStream_t stream = c->sm.stream;
    const int k = (int)(c->n % 3);
    // the upload slot was last read by the copy of frame n - 3
    hipError_t e = c->n >= 3 ? hipEventSynchronize(c->uploaded[k]) : hipSuccess;
    if (e == hipSuccess) e = upload_frame(c->sm, c->slot[k], c->staging[k], c->frame_bytes, *frame, cf.format, cf.H, cf.W);
    if (e == hipSuccess) e = hipEventRecord(c->uploaded[k], stream);
    if (e != hipSuccess) return fail(c, (int)e);
    if (c->n >= 2) {                                                   // frame n - 1 between n - 2 and n
        const fldr_video_frame cur = packed(c->slot[(c->n + 2) % 3], cf.format, cf.H, cf.W);
        const fldr_video_frame prev = packed(c->slot[(c->n + 1) % 3], cf.format, cf.H, cf.W);
        const fldr_video_frame next = packed(c->slot[k], cf.format, cf.H, cf.W);
        const int r = enqueue_measure(cf.H, cf.W, cf.format, &cur, &prev, &next, c->params, c->state_dev, stream);
        if (r) return fail(c, r);
        e = hipMemcpyAsync(&c->ring[c->measured % cf.window], c->state_dev, sizeof(fldr_probe_result), hipMemcpyDeviceToHost, stream);
        if (e != hipSuccess) return fail(c, (int)e);
        c->measured += 1;
    }
    c->n += 1;
    return 0;
}

extern "C" FLDR_PROBE_API int fldr_probe_verdict_get(fldr_probe* c, fldr_probe_verdict* out) {
    if (!c || !out) return FLDR_RATE_E_ARG;
    CK(settle(c));
    fldr_probe_result rs[FLDR_PROBE_MAX_WINDOW];
    const int M = held(c);
    for (int i = 0; i < M; ++i) rs[i] = c->ring[(c->measured - M + i) % c->cfg.window];
    classify(rs, M, c->params, *out);
    return 0;
}

extern "C" FLDR_PROBE_API int fldr_probe_result_get(fldr_probe* c, int i, fldr_probe_result* out, int64_t* frame) {
    if (!c || !out || i < 0 || i >= held(c)) return FLDR_RATE_E_ARG;
    CK(settle(c));
    const int M = held(c);
    if (i >= M) return FLDR_RATE_E_ARG;                                // a failed wait has reset the object
    *out = c->ring[(c->measured - M + i) % c->cfg.window];
    if (frame) *frame = c->measured - M + i + 1;
    return 0;
}

extern "C" FLDR_PROBE_API int fldr_probe_reset(fldr_probe* c) {
    if (!c) return FLDR_RATE_E_ARG;
    DeviceGuard g(c->sm.device);
    if (g.ok) drain(c->sm);
    forget(c);
    return 0;
}

extern "C" FLDR_PROBE_API void fldr_probe_destroy(fldr_probe* c) {
    if (!c) return;
    destroy(c);
}
