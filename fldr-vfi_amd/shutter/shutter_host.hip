// libfldr_shutter.so, host side: validation, accumulate / resolve / mix, fldr_shutter_forward (fldr_video_forward -> mix), the window rule
// (fldr_shutter_plan) and the shutter converter for streams of host frames.  The video API's rules for formats and frames, and the
// stream / device block / pinned block the converter owns, come from ../video/frame_host.h.  The only fldr_* functions called are those
// of fldr_rate.h, fldr_video.h and fldr_model.h.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <vector>

#include "../video/frame_host.h"
#include "shutter_internal.h"

using namespace fldr_shutter_impl;

namespace {

typedef __int128 wide;                 // the window rule's products: exact whatever j is

bool same_format(const fldr_video_format& a, const fldr_video_format& b) {
    return a.layout == b.layout && a.matrix == b.matrix && a.range == b.range && deep(a) == deep(b);
}

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

int check_sources(const fldr_video_format& fmt, int W, const fldr_video_frame* frames, const int32_t* weights, int n) {
    if (!frames || !weights || n < 1) return FLDR_SHUTTER_E_ARG;
    for (int k = 0; k < n; ++k) CK(check_frame(frames[k], fmt, W));
    for (int k = 0; k < n; ++k) if (weights[k] < 1 || weights[k] > 255) return FLDR_SHUTTER_E_WEIGHT;
    return 0;
}

int check_acc(const void* acc) { return !acc || ((uintptr_t)acc & (ALIGN - 1)) ? FLDR_SHUTTER_E_ACC : 0; }

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

int64_t gcd64(int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; }

// the reduced terms of a configuration's window rule
struct Rule {
    int64_t A, B;                      // output j at input position j A / B
    int64_t sn, sd;                    // the shutter
    int64_t sub;
    int max_out;
};

int rule_of(const fldr_shutter_config& c, Rule& r) {
    if (c.sub < 1 || c.sub > FLDR_SHUTTER_MAX_SUB) return FLDR_SHUTTER_E_ARG;
    if (c.in_num <= 0 || c.in_den <= 0 || c.out_num <= 0 || c.out_den <= 0 || c.shutter_num <= 0 || c.shutter_den <= 0) return FLDR_SHUTTER_E_RATIO;
    if (c.shutter_num > c.shutter_den) return FLDR_SHUTTER_E_RATIO;
    r.A = (int64_t)c.in_num * c.out_den; r.B = (int64_t)c.in_den * c.out_num;
    const int64_t g = gcd64(r.A, r.B);
    r.A /= g; r.B /= g;
    const int64_t gs = gcd64(c.shutter_num, c.shutter_den);
    r.sn = c.shutter_num / gs; r.sd = c.shutter_den / gs;
    r.sub = c.sub;
    if (r.A > (1ll << 24) || r.B > (1ll << 24) || r.sd > (1ll << 24)) return FLDR_SHUTTER_E_RATIO;
    const wide len_n = (wide)r.sn * r.A * r.sub, len_d = (wide)r.sd * r.B;      // the window's length in grid points
    if (len_n < len_d) return FLDR_SHUTTER_E_RATIO;                              // it could hold no point
    if ((len_n + len_d - 1) / len_d > FLDR_SHUTTER_MAX_TOTAL) return FLDR_SHUTTER_E_RATIO;
    const int64_t per_push = (r.B + r.A - 1) / r.A + 1;
    if (per_push > FLDR_SHUTTER_MAX_OUT) return FLDR_SHUTTER_E_RATIO;
    r.max_out = (int)per_push;
    return 0;
}

wide ceil_div(wide a, wide b) { return (a + b - 1) / b; }

// m belongs to j iff j A sub sd <= m B sd < j A sub sd + sn A sub
void window(const Rule& r, int64_t j, int64_t& first, int64_t& last) {
    const wide lo = (wide)j * r.A * r.sub * r.sd, hi = lo + (wide)r.sn * r.A * r.sub, step = (wide)r.B * r.sd;
    first = (int64_t)ceil_div(lo, step);
    last = (int64_t)(ceil_div(hi, step) - 1);
}

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
    CK(check_sources(*fmt, W, frames, weights, n));
    CK(check_acc(acc));
    return enqueue_accumulate(g, frames, weights, n, first != 0, acc, (hipStream_t)stream);
}

extern "C" FLDR_SHUTTER_API int fldr_shutter_resolve(int H, int W, const fldr_video_format* fmt, const void* acc, int total,
                                                     const fldr_video_frame* out, void* stream) {
    Geometry g;
    CK(check_size(H, W, fmt, g));
    if (!out) return FLDR_SHUTTER_E_ARG;
    CK(check_frame(*out, *fmt, W));
    if (total < 1 || total > FLDR_SHUTTER_MAX_TOTAL) return FLDR_SHUTTER_E_WEIGHT;
    CK(check_acc(acc));
    return enqueue_resolve(g, acc, total, *out, (hipStream_t)stream);
}

extern "C" FLDR_SHUTTER_API int fldr_shutter_mix(int H, int W, const fldr_video_format* fmt, const fldr_video_frame* frames, const int32_t* weights,
                                                 int n, const fldr_video_frame* out, void* stream) {
    Geometry g;
    CK(check_size(H, W, fmt, g));
    if (n > MAX_FRAMES || !out) return FLDR_SHUTTER_E_ARG;
    CK(check_sources(*fmt, W, frames, weights, n));
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
    if (!io || !w) return FLDR_SHUTTER_E_ARG;
    if (io->H < 2 || io->W < 2 || io->n_t < 1 || !io->t || !io->out) return FLDR_VIDEO_E_ARG;
    if (io->n_t > FLDR_SHUTTER_MAX_SUB) return FLDR_SHUTTER_E_ARG;
    CK(check_format(io->in_format));
    CK(check_format(io->out_format));
    if (!same_format(io->in_format, io->out_format)) return FLDR_SHUTTER_E_FORMAT;
    const fldr_video_format& fmt = io->in_format;
    const int H = io->H, W = io->W, n_t = io->n_t;
    for (int f = 0; f < 2; ++f) CK(check_frame(io->in[f], fmt, W));
    CK(check_frame(io->out[0], fmt, W));
    if (w0 < 0 || w0 > 255 || w1 < 0 || w1 > 255) return FLDR_SHUTTER_E_WEIGHT;
    for (int k = 0; k < n_t; ++k) if (w[k] < 1 || w[k] > 255) return FLDR_SHUTTER_E_WEIGHT;
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
    CK(rule_of(*cfg, r));
    window(r, j, *first, *last);
    return 0;
}

struct fldr_shutter {
    const fldr_model* model;
    fldr_shutter_config cfg;
    Rule rule;
    Geometry geo;
    // device: slot 0, slot 1, sub - 1 sub-frames, max_out outputs, the accumulator, t, scene state, workspace
    // pinned: one input frame, max_out output frames, t, the scene result
    StreamMem sm;
    int64_t frame_bytes, ws_bytes;
    uint8_t* slot[2];
    uint8_t* sub_dev;
    uint8_t* out_dev;
    void* acc;
    float* t_dev;
    void* state_dev;
    void* ws;
    uint8_t* in_host;
    uint8_t* out_host;
    float* t_host;
    fldr_scene_result* scene_host;
    int prev;                          // slot holding the previous frame, -1 when none
    int64_t n;                         // frames pushed since create / reset
    int64_t cuts;                      // cuts seen: the scene of the previous frame
    int64_t j;                         // the first output not yet returned
    int32_t open_points, open_interp;  // of window j, what the accumulator holds (0 points: not begun)
    int64_t open_scene;
};

namespace {

void restart(fldr_shutter* s) { s->prev = -1; s->n = 0; s->cuts = 0; s->j = 0; s->open_points = s->open_interp = 0; s->open_scene = 0; }

// D2H of the first `count` device outputs, one synchronisation, then into the caller's frames
int deliver(fldr_shutter* s, int rc, int count, const fldr_video_frame* host_outs) {
    hipError_t e;
    if (!rc && count) {
        e = hipMemcpyAsync(s->out_host, s->out_dev, (size_t)(count * s->frame_bytes), hipMemcpyDeviceToHost, s->sm.stream);
        if (e != hipSuccess) rc = (int)e;
    }
    e = hipStreamSynchronize(s->sm.stream);
    if (!rc && e != hipSuccess) rc = (int)e;
    if (rc) return rc;
    for (int k = 0; k < count; ++k) unpack_frame(host_outs[k], s->out_host + k * s->frame_bytes, s->cfg.format, s->cfg.H, s->cfg.W);
    return 0;
}

}  // namespace

extern "C" FLDR_SHUTTER_API int fldr_shutter_create(const fldr_model* m, const fldr_shutter_config* cfg, fldr_shutter** out) {
    if (!cfg || !out) return FLDR_SHUTTER_E_ARG;
    *out = nullptr;
    if (cfg->H < 2 || cfg->W < 2 || cfg->device < 0 || (unsigned)cfg->scene > 1u) return FLDR_SHUTTER_E_ARG;
    for (int i = 0; i < 4; ++i) if (cfg->reserved[i]) return FLDR_SHUTTER_E_ARG;
    const fldr_scene_params& sp = cfg->scene_params;
    if (sp.sad_permille < 0 || sp.sad_permille > 1000 || sp.hist_permille < 0 || sp.hist_permille > 1000 || sp.reserved[0] || sp.reserved[1])
        return FLDR_SHUTTER_E_ARG;
    CK(check_format(cfg->format));
    Rule r;
    CK(rule_of(*cfg, r));
    Geometry g;
    if (!geometry(cfg->H, cfg->W, cfg->format, g)) return FLDR_SHUTTER_E_ARG;
    if (!m) return FLDR_SHUTTER_E_ARG;
    const int H = cfg->H, W = cfg->W;
    const int n_sub = cfg->sub - 1;
    const int64_t wsb = fldr_video_workspace_bytes(m, H, W, n_sub > 0 ? n_sub : 1);
    if (wsb < 0) return (int)wsb;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device >= ndev) { (void)hipGetLastError(); return FLDR_SHUTTER_E_DEVICE; }
    fldr_shutter* s = new (std::nothrow) fldr_shutter();
    if (!s) return FLDR_SHUTTER_E_DEVICE;
    s->model = m;
    s->cfg = *cfg;
    s->rule = r;
    s->geo = g;
    restart(s);
    s->frame_bytes = align_up(packed_bytes(cfg->format, H, W));
    s->ws_bytes = align_up(wsb);
    const int64_t t_bytes = align_up(4ll * FLDR_SHUTTER_MAX_SUB), acc_bytes = align_up(4 * g.samples);
    const int64_t dev_total = (2 + n_sub + r.max_out) * s->frame_bytes + acc_bytes + t_bytes + FLDR_SCENE_STATE_BYTES + s->ws_bytes;
    const int64_t host_total = (1 + r.max_out) * s->frame_bytes + t_bytes + ALIGN;
    if (!open_stream_mem(s->sm, cfg->device, dev_total, host_total)) { delete s; return FLDR_SHUTTER_E_DEVICE; }
    s->slot[0] = s->sm.dev;
    s->slot[1] = s->slot[0] + s->frame_bytes;
    s->sub_dev = s->slot[1] + s->frame_bytes;
    s->out_dev = s->sub_dev + n_sub * s->frame_bytes;
    s->acc = s->out_dev + r.max_out * s->frame_bytes;
    s->t_dev = (float*)((char*)s->acc + acc_bytes);
    s->state_dev = (char*)s->t_dev + t_bytes;
    s->ws = (char*)s->state_dev + FLDR_SCENE_STATE_BYTES;
    s->in_host = s->sm.pinned;
    s->out_host = s->in_host + s->frame_bytes;
    s->t_host = (float*)(s->out_host + r.max_out * s->frame_bytes);
    s->scene_host = (fldr_scene_result*)((char*)s->t_host + t_bytes);
    *out = s;
    return 0;
}

extern "C" FLDR_SHUTTER_API int fldr_shutter_max_out(const fldr_shutter* s) { return s ? s->rule.max_out : FLDR_SHUTTER_E_ARG; }

extern "C" FLDR_SHUTTER_API int fldr_shutter_push(fldr_shutter* s, const fldr_video_frame* frame, const fldr_video_frame* host_outs,
                                                  fldr_shutter_info* info, int* n_out, fldr_scene_result* scene) {
    if (!s || !frame || !n_out) return FLDR_SHUTTER_E_ARG;
    *n_out = 0;
    if (scene) memset(scene, 0, sizeof(*scene));
    const fldr_shutter_config& c = s->cfg;
    const Rule& r = s->rule;
    const int H = c.H, W = c.W;
    const int sub = c.sub;
    const fldr_video_format& fmt = c.format;
    CK(check_frame(*frame, fmt, W));
    // the points this push supplies, and how many outputs can end in it at the most: every window begun at or before frame n
    const bool pair = s->prev >= 0;
    const int64_t hi = s->n * sub, lo = pair ? hi - sub + 1 : hi;
    int possible = 0;
    for (int64_t j = s->j; possible < r.max_out; ++j) {
        int64_t f, l;
        window(r, j, f, l);
        if (f > hi) break;
        ++possible;
    }
    if (possible) {
        if (!host_outs) return FLDR_SHUTTER_E_ARG;
        for (int k = 0; k < possible; ++k) CK(check_frame(host_outs[k], fmt, W));
    }
    DeviceGuard guard(s->sm.device);
    if (!guard.ok) return FLDR_SHUTTER_E_DEVICE;
    const hipStream_t stream = s->sm.stream;
    const int cur = s->prev == 0 ? 1 : 0;                          // the slot not holding the previous frame
    hipError_t e = upload_frame(s->sm, s->slot[cur], s->in_host, s->frame_bytes, *frame, fmt, H, W);
    int rc = e == hipSuccess ? 0 : (int)e;
    fldr_video_frame in[2] = { packed(s->slot[pair ? s->prev : cur], fmt, H, W), packed(s->slot[cur], fmt, H, W) };
    // the cut flag of the pair, on the host before the pair is planned
    bool cut = false;
    if (!rc && pair && c.scene == 1) {
        rc = fldr_scene_measure(H, W, &fmt, in, &c.scene_params, s->state_dev, stream);
        if (!rc) {
            e = hipMemcpyAsync(s->scene_host, s->state_dev, sizeof(fldr_scene_result), hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
            if (e != hipSuccess) rc = (int)e;
        }
        if (!rc) cut = s->scene_host->cut != 0;
    }
    if (rc) { (void)hipStreamSynchronize(stream); restart(s); return rc; }
    // ---- the plan: per window, the weight of frame n - 1, of frame n and of each sub-frame k = 1 .. sub - 1 ----
    struct Step { int64_t j; int w_prev, w_cur; uint8_t w_sub[FLDR_SHUTTER_MAX_SUB]; int points, interp; bool begins, ends, truncated; };
    std::vector<Step> steps;
    bool wanted[FLDR_SHUTTER_MAX_SUB] = { false };
    int64_t j = s->j;
    int open_points = s->open_points, open_interp = s->open_interp;
    int64_t open_scene = s->open_scene;
    while ((int)steps.size() < r.max_out) {
        int64_t f, l;
        window(r, j, f, l);
        if (f > hi) break;
        Step st;
        memset(&st, 0, sizeof(st));
        st.j = j;
        st.begins = open_points == 0;
        const int64_t from = f > lo ? f : lo, to = l < hi ? l : hi;
        for (int64_t m = from; m <= to; ++m) {
            const int k = pair ? (int)(m - (hi - sub)) : sub;          // 1 .. sub; sub: the pushed frame itself
            const int64_t sc = s->cuts + ((cut && 2 * k >= sub) ? 1 : 0);
            if (open_points + st.points == 0) open_scene = sc;        // the window's first point names its scene
            if (sc != open_scene) { st.truncated = true; break; }
            ++st.points;
            if (k == sub) ++st.w_cur;
            else if (cut) ++(2 * k < sub ? st.w_prev : st.w_cur);
            else { ++st.w_sub[k]; ++st.interp; wanted[k] = true; }
        }
        st.ends = st.truncated || l <= hi;
        open_points += st.points;
        open_interp += st.interp;
        st.points = open_points;
        st.interp = open_interp;
        steps.push_back(st);
        if (!st.ends) break;
        open_points = open_interp = 0;
        ++j;
    }
    // ---- one forward with exactly the sub-times some window keeps ----
    int slot_of[FLDR_SHUTTER_MAX_SUB], n_t = 0;
    for (int k = 1; k < sub; ++k) if (wanted[k]) { slot_of[k] = n_t; s->t_host[n_t++] = (float)k / (float)sub; }
    if (n_t) {
        e = hipMemcpyAsync(s->t_dev, s->t_host, 4ull * n_t, hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) rc = (int)e;
        std::vector<fldr_video_frame> subs((size_t)n_t);
        for (int k = 0; k < n_t; ++k) subs[k] = packed(s->sub_dev + k * s->frame_bytes, fmt, H, W);
        fldr_video_io io;
        memset(&io, 0, sizeof(io));
        io.H = H; io.W = W;
        io.in_format = io.out_format = fmt;
        io.in[0] = in[0]; io.in[1] = in[1];
        io.n_t = n_t; io.t = s->t_dev; io.out = subs.data();
        if (!rc) rc = fldr_video_forward(s->model, &io, s->ws, s->ws_bytes, stream);
    }
    // ---- the windows, in order, on the one accumulator ----
    int count = 0;
    for (size_t q = 0; q < steps.size() && !rc; ++q) {
        const Step& st = steps[q];
        fldr_video_frame frames[MAX_FRAMES];
        int32_t weights[MAX_FRAMES];
        int nf = 0;
        if (st.w_prev) { frames[nf] = in[0]; weights[nf++] = st.w_prev; }
        for (int k = 1; k < sub; ++k)
            if (st.w_sub[k]) { frames[nf] = packed(s->sub_dev + slot_of[k] * s->frame_bytes, fmt, H, W); weights[nf++] = st.w_sub[k]; }
        if (st.w_cur) { frames[nf] = in[1]; weights[nf++] = st.w_cur; }
        const fldr_video_frame out = packed(s->out_dev + count * s->frame_bytes, fmt, H, W);
        if (st.begins && st.ends) {
            rc = enqueue_mix(s->geo, frames, weights, nf, out, stream);         // begins with a point of this push: nf >= 1
        } else {
            if (nf) rc = enqueue_accumulate(s->geo, frames, weights, nf, st.begins, s->acc, stream);
            if (!rc && st.ends) rc = enqueue_resolve(s->geo, s->acc, st.points, out, stream);
        }
        if (st.ends) {
            if (info) { fldr_shutter_info i = { st.j, st.points, st.interp, st.truncated ? 1 : 0, 0 }; info[count] = i; }
            ++count;
        }
    }
    rc = deliver(s, rc, count, host_outs);
    if (rc) { restart(s); return rc; }     // the held frame and the accumulator are not to be trusted: as after a reset
    if (pair && c.scene == 1 && scene) *scene = *s->scene_host;
    *n_out = count;
    s->j = j;
    s->open_points = open_points; s->open_interp = open_interp; s->open_scene = open_scene;
    if (cut) s->cuts += 1;
    s->n += 1;
    s->prev = cur;
    return 0;
}

extern "C" FLDR_SHUTTER_API int fldr_shutter_flush(fldr_shutter* s, const fldr_video_frame* host_outs, fldr_shutter_info* info, int* n_out) {
    if (!s || !n_out) return FLDR_SHUTTER_E_ARG;
    *n_out = 0;
    if (s->open_points == 0) return 0;
    if (!host_outs) return FLDR_SHUTTER_E_ARG;
    const fldr_shutter_config& c = s->cfg;
    CK(check_frame(host_outs[0], c.format, c.W));
    DeviceGuard guard(s->sm.device);
    if (!guard.ok) return FLDR_SHUTTER_E_DEVICE;
    int rc = enqueue_resolve(s->geo, s->acc, s->open_points, packed(s->out_dev, c.format, c.H, c.W), s->sm.stream);
    rc = deliver(s, rc, 1, host_outs);
    if (rc) { restart(s); return rc; }
    if (info) { fldr_shutter_info i = { s->j, s->open_points, s->open_interp, 1, 0 }; info[0] = i; }
    s->j += 1;
    s->open_points = s->open_interp = 0;
    *n_out = 1;
    return 0;
}

extern "C" FLDR_SHUTTER_API int fldr_shutter_reset(fldr_shutter* s) {
    if (!s) return FLDR_SHUTTER_E_ARG;
    restart(s);
    return 0;
}

extern "C" FLDR_SHUTTER_API void fldr_shutter_destroy(fldr_shutter* s) {
    if (s) { close_stream_mem(s->sm); delete s; }
}
