// libfldr_shutter.so, host side: validation, accumulate / resolve / mix, fldr_shutter_forward (fldr_video_forward -> mix), and the public
// face of the window rule (fldr_shutter_plan) and of the shutter converter for streams of host frames.  The rule and the converter
// themselves are in session_host.h (shared with libfldr_light.so, with the checks both libraries make alike: the sources, the alignment
// of a block, the forward's refusals), which this file hands its three integration calls; the video API's
// rules for formats and frames, and the stream / device block / pinned block the converter owns, come from ../video/frame_host.h.  The
// only fldr_* functions called are those of fldr_rate.h, fldr_video.h and fldr_model.h.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <vector>

#include "../video/frame_host.h"
#include "session_host.h"
#include "shutter_internal.h"

using namespace fldr_shutter_impl;

namespace {

bool aligned16(const fldr_video_frame& f, int np) {
    uintptr_t bits = 0;
    for (int p = 0; p < np; ++p) bits |= (uintptr_t)f.plane[p] | (uintptr_t)f.pitch[p];
    return (bits & 15) == 0;
}

int check_size(int H, int W, const fldr_video_format* fmt, Geometry& g) {
    if (!fmt || H < 1 || W < 1) return FLDR_SHUTTER_E_ARG;
    CK(check_format(*fmt));
    return geometry(H, W, *fmt, g) ? 0 : FLDR_SHUTTER_E_ARG;
}

// frames[k0 .. k0 + n) as one launch reads them; -> whether all of them take the wide form
bool fill_sources(Sources& s, const Geometry& g, const fldr_video_frame* frames, const int32_t* weights, int n) {
    memset(&s, 0, sizeof(s));
    bool vec = true;
    for (int k = 0; k < n; ++k) {
        for (int p = 0; p < g.np; ++p) { s.plane[k][p] = (const uint8_t*)frames[k].plane[p]; s.pitch[k][p] = frames[k].pitch[p]; }
        s.weight[k] = (uint32_t)weights[k];
        vec = vec && aligned16(frames[k], g.np);
    }
    s.n = n;
    return vec;
}

bool fill_target(Target& t, const Geometry& g, const fldr_video_frame& out, int total) {
    memset(&t, 0, sizeof(t));
    for (int p = 0; p < g.np; ++p) { t.plane[p] = (uint8_t*)out.plane[p]; t.pitch[p] = out.pitch[p]; }
    t.total = (uint32_t)total;
    reciprocal(t.total, t.mul, t.shift);
    t.maxv = g.mode == S_BYTE ? 255u : 1023u;
    return aligned16(out, g.np);
}

// validated arguments -> launches
int enqueue_accumulate(const Geometry& g, const fldr_video_frame* frames, const int32_t* weights, int n, bool first, void* acc, hipStream_t s) {
    Sources src;
    for (int k0 = 0; k0 < n; k0 += MAX_FRAMES) {
        const int m = n - k0 < MAX_FRAMES ? n - k0 : MAX_FRAMES;
        const bool vec = fill_sources(src, g, frames + k0, weights + k0, m);
        CK(launch_accumulate(g, src, first && k0 == 0, (uint32_t*)acc, vec, s));
    }
    return 0;
}

int enqueue_resolve(const Geometry& g, const void* acc, int total, const fldr_video_frame& out, hipStream_t s) {
    Target t;
    const bool vec = fill_target(t, g, out, total);
    return launch_resolve(g, (const uint32_t*)acc, t, vec, s);
}

int enqueue_mix(const Geometry& g, const fldr_video_frame* frames, const int32_t* weights, int n, const fldr_video_frame& out, hipStream_t s) {
    Sources src;
    Target t;
    int total = 0;
    for (int k = 0; k < n; ++k) total += weights[k];
    const bool vs = fill_sources(src, g, frames, weights, n), vt = fill_target(t, g, out, total);
    return launch_mix(g, src, t, vs && vt, s);
}

// the three calls as the converter of session_host.h takes them
int op_check(void*, int H, int W, const fldr_video_format& fmt) {
    Geometry g;
    return geometry(H, W, fmt, g) ? 0 : FLDR_SHUTTER_E_ARG;
}

int64_t op_acc_bytes(int H, int W, const fldr_video_format& fmt) {
    Geometry g;
    geometry(H, W, fmt, g);
    return align_up(4 * g.samples);
}

int64_t op_scratch_bytes(int, int, const fldr_video_format&) { return 0; }

int op_accumulate(void*, int H, int W, const fldr_video_format& fmt, const fldr_video_frame* frames, const int32_t* weights, int n, bool first,
                  void* acc, void*, hipStream_t s) {
    Geometry g;
    geometry(H, W, fmt, g);
    return enqueue_accumulate(g, frames, weights, n, first, acc, s);
}

int op_resolve(void*, int H, int W, const fldr_video_format& fmt, const void* acc, int total, const fldr_video_frame& out, void*, hipStream_t s) {
    Geometry g;
    geometry(H, W, fmt, g);
    return enqueue_resolve(g, acc, total, out, s);
}

int op_mix(void*, int H, int W, const fldr_video_format& fmt, const fldr_video_frame* frames, const int32_t* weights, int n,
           const fldr_video_frame& out, void*, hipStream_t s) {
    Geometry g;
    geometry(H, W, fmt, g);
    return enqueue_mix(g, frames, weights, n, out, s);
}

const Integration INTEGER_MEAN = { nullptr, FLDR_SHUTTER_E_ARG, FLDR_SHUTTER_E_RATIO, FLDR_SHUTTER_E_DEVICE, FLDR_SHUTTER_MAX_TOTAL, false,
                                   op_check, op_acc_bytes, op_scratch_bytes, op_accumulate, op_resolve, op_mix };

}  // namespace

extern "C" FLDR_SHUTTER_API int fldr_shutter_version(void) { return FLDR_SHUTTER_VERSION; }

extern "C" FLDR_SHUTTER_API const char* fldr_shutter_error_string(int code) {
    switch (code) {
    case 0: return "success";
    case FLDR_SHUTTER_E_ARG: return "fldr_shutter: bad argument";
    case FLDR_SHUTTER_E_FORMAT: return "fldr_shutter: in_format and out_format differ";
    case FLDR_SHUTTER_E_ACC: return "fldr_shutter: accumulator missing or misaligned";
    case FLDR_SHUTTER_E_WEIGHT: return "fldr_shutter: a weight or a total outside its range";
    case FLDR_SHUTTER_E_RATIO: return "fldr_shutter: rate or shutter terms outside what the converter takes";
    case FLDR_SHUTTER_E_DEVICE: return "fldr_shutter: no such device or out of memory";
    default: return code > -300 ? fldr_rate_error_string(code) : "fldr_shutter: unknown error";
    }
}

extern "C" FLDR_SHUTTER_API int fldr_shutter_sizeof(int which) {
    switch (which) {
    case 0: return (int)sizeof(fldr_shutter_config);
    case 1: return (int)sizeof(fldr_shutter_info);
    default: return FLDR_SHUTTER_E_ARG;
    }
}

extern "C" FLDR_SHUTTER_API int64_t fldr_shutter_acc_bytes(int H, int W, const fldr_video_format* fmt) {
    Geometry g;
    const int rc = check_size(H, W, fmt, g);
    return rc ? rc : align_up(4 * g.samples);
}

extern "C" FLDR_SHUTTER_API int fldr_shutter_accumulate(int H, int W, const fldr_video_format* fmt, const fldr_video_frame* frames,
                                                        const int32_t* weights, int n, int first, void* acc, void* stream) {
    Geometry g;
    CK(check_size(H, W, fmt, g));
    CK(check_sources(*fmt, W, frames, weights, n, FLDR_SHUTTER_E_ARG, FLDR_SHUTTER_E_WEIGHT, 0));
    CK(check_aligned(acc, FLDR_SHUTTER_E_ACC));
    return enqueue_accumulate(g, frames, weights, n, first != 0, acc, (hipStream_t)stream);
}

extern "C" FLDR_SHUTTER_API int fldr_shutter_resolve(int H, int W, const fldr_video_format* fmt, const void* acc, int total,
                                                     const fldr_video_frame* out, void* stream) {
    Geometry g;
    CK(check_size(H, W, fmt, g));
    if (!out) return FLDR_SHUTTER_E_ARG;
    CK(check_frame(*out, *fmt, W));
    if (total < 1 || total > FLDR_SHUTTER_MAX_TOTAL) return FLDR_SHUTTER_E_WEIGHT;
    CK(check_aligned(acc, FLDR_SHUTTER_E_ACC));
    return enqueue_resolve(g, acc, total, *out, (hipStream_t)stream);
}

extern "C" FLDR_SHUTTER_API int fldr_shutter_mix(int H, int W, const fldr_video_format* fmt, const fldr_video_frame* frames, const int32_t* weights,
                                                 int n, const fldr_video_frame* out, void* stream) {
    Geometry g;
    CK(check_size(H, W, fmt, g));
    if (n > MAX_FRAMES || !out) return FLDR_SHUTTER_E_ARG;
    CK(check_sources(*fmt, W, frames, weights, n, FLDR_SHUTTER_E_ARG, FLDR_SHUTTER_E_WEIGHT, 0));
    CK(check_frame(*out, *fmt, W));
    return enqueue_mix(g, frames, weights, n, *out, (hipStream_t)stream);
}

extern "C" FLDR_SHUTTER_API int fldr_shutter_reciprocal(int total, uint32_t* mul, uint32_t* shift) {
    if (!mul || !shift) return FLDR_SHUTTER_E_ARG;
    if (total < 1 || total > FLDR_SHUTTER_MAX_TOTAL) return FLDR_SHUTTER_E_WEIGHT;
    reciprocal((uint32_t)total, *mul, *shift);
    return 0;
}

// ---- one pair ---------------------------------------------------------------------------------------------------------------------------
namespace {

int64_t scratch_frame_bytes(int H, int W) {                 // a packed frame of any of the four formats
    const int64_t ch = (H + 1) / 2, cw = (W + 1) / 2;
    return align_up(2 * ((int64_t)H * W + 2 * ch * cw));
}

}  // namespace

extern "C" FLDR_SHUTTER_API int64_t fldr_shutter_workspace_bytes(const fldr_model* m, int H, int W, int n_t) {
    const int64_t vb = fldr_video_workspace_bytes(m, H, W, n_t);
    return vb < 0 ? vb : align_up(vb) + n_t * scratch_frame_bytes(H, W);
}

extern "C" FLDR_SHUTTER_API int fldr_shutter_forward(const fldr_model* m, const fldr_video_io* io, int w0, int w1, const int32_t* w, void* ws,
                                                     int64_t ws_bytes, void* stream) {
    // everything fldr_video_forward and the mix would refuse is refused here, before anything is enqueued
    int total;
    CK(forward_preamble(io, w0, w1, w, FLDR_SHUTTER_E_ARG, FLDR_SHUTTER_E_FORMAT, FLDR_SHUTTER_E_WEIGHT, 0, &total));
    const fldr_video_format& fmt = io->in_format;
    const int H = io->H, W = io->W, n_t = io->n_t;
    Geometry g;
    if (!geometry(H, W, fmt, g)) return FLDR_SHUTTER_E_ARG;
    const int64_t vb = fldr_video_workspace_bytes(m, H, W, n_t);
    if (vb < 0) return (int)vb;
    const int64_t sub_off = align_up(vb), fb = scratch_frame_bytes(H, W);
    if (!ws || ((uintptr_t)ws & (ALIGN - 1)) || ws_bytes < sub_off + n_t * fb) return FLDR_VIDEO_E_WORKSPACE;
    fldr_video_frame frames[MAX_FRAMES];
    int32_t weights[MAX_FRAMES];
    int n = 0;
    if (w0) { frames[n] = io->in[0]; weights[n++] = w0; }
    if (w1) { frames[n] = io->in[1]; weights[n++] = w1; }
    std::vector<fldr_video_frame> subs((size_t)n_t);
    for (int k = 0; k < n_t; ++k) {
        subs[k] = packed((uint8_t*)ws + sub_off + k * fb, fmt, H, W);
        frames[n] = subs[k]; weights[n++] = w[k];
    }
    fldr_video_io inner = *io;
    inner.out = subs.data();
    CK(fldr_video_forward(m, &inner, ws, sub_off, stream));
    return enqueue_mix(g, frames, weights, n, io->out[0], (hipStream_t)stream);
}

// ---- the converter ------------------------------------------------------------------------------------------------------------------------
extern "C" FLDR_SHUTTER_API int fldr_shutter_plan(const fldr_shutter_config* cfg, int64_t j, int64_t* first, int64_t* last) {
    if (!cfg || !first || !last || j < 0) return FLDR_SHUTTER_E_ARG;
    Rule r;
    CK(rule_of(*cfg, r, FLDR_SHUTTER_E_ARG, FLDR_SHUTTER_E_RATIO, FLDR_SHUTTER_MAX_TOTAL));
    window(r, j, *first, *last);
    return 0;
}

struct fldr_shutter { Session s; };

extern "C" FLDR_SHUTTER_API int fldr_shutter_create(const fldr_model* m, const fldr_shutter_config* cfg, fldr_shutter** out) {
    if (!cfg || !out) return FLDR_SHUTTER_E_ARG;
    *out = nullptr;
    fldr_shutter* h = new (std::nothrow) fldr_shutter();
    if (!h) return FLDR_SHUTTER_E_DEVICE;
    const int rc = session_open(&h->s, m, cfg, INTEGER_MEAN);
    if (rc) { delete h; return rc; }
    *out = h;
    return 0;
}

extern "C" FLDR_SHUTTER_API int fldr_shutter_max_out(const fldr_shutter* h) { return h ? h->s.rule.max_out : FLDR_SHUTTER_E_ARG; }

extern "C" FLDR_SHUTTER_API int fldr_shutter_push(fldr_shutter* h, const fldr_video_frame* frame, const fldr_video_frame* host_outs,
                                                  fldr_shutter_info* info, int* n_out, fldr_scene_result* scene) {
    if (!h || !frame || !n_out) return FLDR_SHUTTER_E_ARG;
    return session_push(&h->s, frame, host_outs, info, n_out, scene);
}

extern "C" FLDR_SHUTTER_API int fldr_shutter_flush(fldr_shutter* h, const fldr_video_frame* host_outs, fldr_shutter_info* info, int* n_out) {
    if (!h || !n_out) return FLDR_SHUTTER_E_ARG;
    return session_flush(&h->s, host_outs, info, n_out);
}

extern "C" FLDR_SHUTTER_API int fldr_shutter_reset(fldr_shutter* h) {
    if (!h) return FLDR_SHUTTER_E_ARG;
    session_restart(&h->s);
    return 0;
}

extern "C" FLDR_SHUTTER_API void fldr_shutter_destroy(fldr_shutter* h) {
    if (h) { close_stream_mem(h->s.sm); delete h; }
}
