// libfldr_cadence.so, host side: validation, fldr_repeat_measure, and the cadence stream (container frames in, the repeats of every
// cycle dropped, the survivors pushed into an inner fldr_rate).  The video API's rules for formats and frames, and the stream / device
// block / pinned block the object owns, come from ../video/frame_host.h; the inner converter's configuration rules come from
// ../rate/rate_plan.h, the checks of a luma tile measure from ../rate/tile_measure_host.h, and the cycle stream — the create prelude,
// the drop selection, the survivors' push, flush, reset — from ../rate/cycle_stream_host.h, which includes them all.  What is here is
// what a push uploads and measures and how its blocks are laid out.  The only fldr_* functions called are those of fldr_rate.h,
// fldr_video.h and fldr_model.h.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../rate/cycle_stream_host.h"
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
    if (!fmt || !in || !tiles_ok(H, W, FLDR_REPEAT_TILE)) return FLDR_CADENCE_E_ARG;
    int rc = resolve_params(p, tile_sad_min);
    if (!rc) rc = check_format(*fmt);
    for (int f = 0; f < 2 && !rc; ++f) rc = check_frame(in[f], *fmt, W);
    if (rc) return rc;
    return check_state(state, FLDR_CADENCE_E_STATE);
}

int enqueue_measure(int H, int W, const fldr_video_format& fmt, const fldr_video_frame in[2], int tile_sad_min, void* state, hipStream_t s) {
    return repeat_measure(in[0].plane[0], in[0].pitch[0], in[1].plane[0], in[1].pitch[0], H, W, luma_mode(deep(fmt), fmt.layout), tile_sad_min,
                          state, s);
}

// the cycle stream's view of this library (../rate/cycle_stream_host.h)
struct CadenceCycle {
    using Config = fldr_cadence_config;
    using Result = fldr_repeat_result;
    using Report = fldr_cadence_report;
    static constexpr int E_ARG = FLDR_CADENCE_E_ARG, E_DEVICE = FLDR_CADENCE_E_DEVICE, MAX_CYCLE = FLDR_CADENCE_MAX_CYCLE;
    // (max_tile_sad, sad) of a before that of b
    static bool key_less(const Result& a, const Result& b) { return a.max_tile_sad != b.max_tile_sad ? a.max_tile_sad < b.max_tile_sad : a.sad < b.sad; }
    static bool report_frame(Report&, int, const Result& res) { return !res.repeat; }
};

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
struct fldr_cadence : CycleStream<CadenceCycle> {
    // device: slot 0, slot 1, the repeat state.  pinned: the ring of `cycle` packed frames as they came, then the `cycle` results.
    uint8_t* slot[2];
    void* state_dev;
    int prev;                          // slot holding the previous frame, -1 when none
    void forget_own() { prev = -1; }
};

extern "C" FLDR_CADENCE_API int fldr_cadence_inner_rate(const fldr_cadence_config* cfg, int32_t* num, int32_t* den) {
    return inner_rate_entry<CadenceCycle>(cfg, num, den);
}

extern "C" FLDR_CADENCE_API int fldr_cadence_create(const fldr_model* m, const fldr_cadence_config* ccfg, fldr_cadence** out) {
    return cycle_create<CadenceCycle>(m, ccfg, out,
        [](const fldr_cadence_config& cc) {
            int tile_sad_min;
            CK(resolve_params(&cc.repeat, tile_sad_min));
            return cc.reserved[0] || cc.reserved[1] ? FLDR_CADENCE_E_ARG : 0;
        },
        [](fldr_cadence* c) {
            const int cycle = c->cfg.cycle;
            const int64_t dev_total = 2 * c->frame_bytes + FLDR_REPEAT_STATE_BYTES;
            const int64_t host_total = cycle * c->frame_bytes + align_up(cycle * RESULT_BYTES);
            if (!open_stream_mem(c->sm, c->cfg.rate.device, dev_total, host_total)) return false;
            c->slot[0] = c->sm.dev;
            c->slot[1] = c->slot[0] + c->frame_bytes;
            c->state_dev = c->slot[1] + c->frame_bytes;
            c->ring = c->sm.pinned;
            c->result_host = (fldr_repeat_result*)(c->ring + cycle * c->frame_bytes);
            return true;
        });
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
    if (completes) CK(check_outs<CadenceCycle>(c, host_outs));
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
    if (r) return fail(c, r);
    c->prev = cur;
    c->n += 1;
    c->m += 1;
    return completes ? finish_cycle<CadenceCycle>(c, c->n - c->m, c->cfg.drop, host_outs, n_out, report) : 0;
}

extern "C" FLDR_CADENCE_API int fldr_cadence_flush(fldr_cadence* c, const fldr_video_frame* host_outs, int* n_out, fldr_cadence_report* report) {
    return cycle_flush<CadenceCycle>(c, host_outs, n_out, report, [](fldr_cadence*) { return 0; });
}

extern "C" FLDR_CADENCE_API int fldr_cadence_reset(fldr_cadence* c) { return cycle_reset<CadenceCycle>(c); }

extern "C" FLDR_CADENCE_API void fldr_cadence_destroy(fldr_cadence* c) { cycle_destroy(c); }
