// The window rule and the converter of include/fldr_shutter.h: which grid points an output keeps, which push returns it, the one forward
// of a push and the windows on one accumulator.  Included by shutter_host.hip and by ../light/light_host.hip: libfldr_light.so plans exactly
// as libfldr_shutter.so because both compile this text.  How points are summed and resolved is the including library's: a small struct of
// integration operations (Integration).  What the kernel entry points and the forward of both libraries check alike is here too, each
// taking the including library's codes: same_format, check_aligned, check_sources and forward_preamble.  Everything is in the unnamed
// namespace: nothing here becomes a symbol of either library.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../video/frame_host.h"
#include "fldr_shutter.h"

namespace {

// accumulate / resolve / mix of device frames in one format and size, their buffers, and what the including library calls its errors
struct Integration {
    void* ctx;                         // the operations' own (a curve)
    int e_arg, e_ratio, e_device;      // the library's codes
    int64_t max_points;                // the largest window create takes
    bool lone_input_unchanged;         // a window of one point that is an input frame returns that frame's bytes
    int (*check)(void* ctx, int H, int W, const fldr_video_format& fmt);      // what the operations refuse about a size and format
    int64_t (*acc_bytes)(int H, int W, const fldr_video_format& fmt);          // a multiple of ALIGN
    int64_t (*scratch_bytes)(int H, int W, const fldr_video_format& fmt);      // a multiple of ALIGN, may be 0
    int (*accumulate)(void* ctx, int H, int W, const fldr_video_format& fmt, const fldr_video_frame* frames, const int32_t* weights, int n,
                      bool first, void* acc, void* scratch, hipStream_t s);
    int (*resolve)(void* ctx, int H, int W, const fldr_video_format& fmt, const void* acc, int total, const fldr_video_frame& out,
                   void* scratch, hipStream_t s);
    int (*mix)(void* ctx, int H, int W, const fldr_video_format& fmt, const fldr_video_frame* frames, const int32_t* weights, int n,
               const fldr_video_frame& out, void* scratch, hipStream_t s);
};

// ---- what accumulate / resolve / mix and the forward of either library refuse alike ----
bool same_format(const fldr_video_format& a, const fldr_video_format& b) {
    return a.layout == b.layout && a.matrix == b.matrix && a.range == b.range && deep(a) == deep(b);
}

// an accumulator or scratch block: present and ALIGN-aligned, else the caller's code
int check_aligned(const void* p, int code) { return !p || ((uintptr_t)p & (ALIGN - 1)) ? code : 0; }

// frames present, every frame valid for the format, every weight in 1 .. 255, and their total <= max_total (0: no bound)
int check_sources(const fldr_video_format& fmt, int W, const fldr_video_frame* frames, const int32_t* weights, int n, int e_arg, int e_weight,
                  int64_t max_total) {
    if (!frames || !weights || n < 1) return e_arg;
    for (int k = 0; k < n; ++k) CK(check_frame(frames[k], fmt, W));
    int64_t total = 0;
    for (int k = 0; k < n; ++k) {
        if (weights[k] < 1 || weights[k] > 255) return e_weight;
        total += weights[k];
    }
    return max_total && total > max_total ? e_weight : 0;
}

// What a forward refuses before it looks at its own geometry, in the order fldr_shutter_forward and fldr_light_forward document: everything
// fldr_video_forward and the mix would refuse about io and the weights.  max_total as in check_sources; *total = w0 + w1 + the sum of w.
int forward_preamble(const fldr_video_io* io, int w0, int w1, const int32_t* w, int e_arg, int e_format, int e_weight, int64_t max_total,
                     int* total) {
    if (!io || !w) return e_arg;
    if (io->H < 2 || io->W < 2 || io->n_t < 1 || !io->t || !io->out) return FLDR_VIDEO_E_ARG;
    if (io->n_t > FLDR_SHUTTER_MAX_SUB) return e_arg;
    CK(check_format(io->in_format));
    CK(check_format(io->out_format));
    if (!same_format(io->in_format, io->out_format)) return e_format;
    for (int f = 0; f < 2; ++f) CK(check_frame(io->in[f], io->in_format, io->W));
    CK(check_frame(io->out[0], io->in_format, io->W));
    if (w0 < 0 || w0 > 255 || w1 < 0 || w1 > 255) return e_weight;
    *total = w0 + w1;
    for (int k = 0; k < io->n_t; ++k) {
        if (w[k] < 1 || w[k] > 255) return e_weight;
        *total += w[k];
    }
    return max_total && *total > max_total ? e_weight : 0;
}

typedef __int128 wide;                 // the window rule's products: exact whatever j is

int64_t gcd64(int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; }

// the reduced terms of a configuration's window rule
struct Rule {
    int64_t A, B;                      // output j at input position j A / B
    int64_t sn, sd;                    // the shutter
    int64_t sub;
    int max_out;
};

int rule_of(const fldr_shutter_config& c, Rule& r, int e_arg, int e_ratio, int64_t max_points) {
    if (c.sub < 1 || c.sub > FLDR_SHUTTER_MAX_SUB) return e_arg;
    if (c.in_num <= 0 || c.in_den <= 0 || c.out_num <= 0 || c.out_den <= 0 || c.shutter_num <= 0 || c.shutter_den <= 0) return e_ratio;
    if (c.shutter_num > c.shutter_den) return e_ratio;
    r.A = (int64_t)c.in_num * c.out_den; r.B = (int64_t)c.in_den * c.out_num;
    const int64_t g = gcd64(r.A, r.B);
    r.A /= g; r.B /= g;
    const int64_t gs = gcd64(c.shutter_num, c.shutter_den);
    r.sn = c.shutter_num / gs; r.sd = c.shutter_den / gs;
    r.sub = c.sub;
    if (r.A > (1ll << 24) || r.B > (1ll << 24) || r.sd > (1ll << 24)) return e_ratio;
    const wide len_n = (wide)r.sn * r.A * r.sub, len_d = (wide)r.sd * r.B;      // the window's length in grid points
    if (len_n < len_d) return e_ratio;                                           // it could hold no point
    if ((len_n + len_d - 1) / len_d > max_points) return e_ratio;
    const int64_t per_push = (r.B + r.A - 1) / r.A + 1;
    if (per_push > FLDR_SHUTTER_MAX_OUT) return e_ratio;
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

struct Session {
    const fldr_model* model;
    fldr_shutter_config cfg;
    Integration op;
    Rule rule;
    // device: slot 0, slot 1, sub - 1 sub-frames, max_out outputs, the accumulator, scratch, t, scene state, workspace
    // pinned: one input frame, max_out output frames, t, the scene result
    StreamMem sm;
    int64_t frame_bytes, ws_bytes;
    uint8_t* slot[2];
    uint8_t* sub_dev;
    uint8_t* out_dev;
    void* acc;
    void* scratch;
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
    int open_lone;                     // the slot of the open window's one point when that is an input frame, else -1
};

void session_restart(Session* s) {
    s->prev = -1; s->n = 0; s->cuts = 0; s->j = 0; s->open_points = s->open_interp = 0; s->open_scene = 0; s->open_lone = -1;
}

// D2H of the first `count` device outputs, one synchronisation, then into the caller's frames
int session_deliver(Session* s, int rc, int count, const fldr_video_frame* host_outs) {
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

// a packed frame on the device -> a packed output slot, byte for byte
int session_copy_frame(Session* s, const uint8_t* from, uint8_t* to) {
    const hipError_t e = hipMemcpyAsync(to, from, (size_t)packed_bytes(s->cfg.format, s->cfg.H, s->cfg.W), hipMemcpyDeviceToDevice, s->sm.stream);
    return e == hipSuccess ? 0 : (int)e;
}

// Validates cfg in the order fldr_shutter_create documents and fills *s (zero-initialised by the caller); the model comes last of the
// host-only checks, the device after it.
int session_open(Session* s, const fldr_model* m, const fldr_shutter_config* cfg, const Integration& op) {
    if (cfg->H < 2 || cfg->W < 2 || cfg->device < 0 || (unsigned)cfg->scene > 1u) return op.e_arg;
    for (int i = 0; i < 4; ++i) if (cfg->reserved[i]) return op.e_arg;
    const fldr_scene_params& sp = cfg->scene_params;
    if (sp.sad_permille < 0 || sp.sad_permille > 1000 || sp.hist_permille < 0 || sp.hist_permille > 1000 || sp.reserved[0] || sp.reserved[1])
        return op.e_arg;
    CK(check_format(cfg->format));
    Rule r;
    CK(rule_of(*cfg, r, op.e_arg, op.e_ratio, op.max_points));
    CK(op.check(op.ctx, cfg->H, cfg->W, cfg->format));
    if (!m) return op.e_arg;
    const int H = cfg->H, W = cfg->W;
    const int n_sub = cfg->sub - 1;
    const int64_t wsb = fldr_video_workspace_bytes(m, H, W, n_sub > 0 ? n_sub : 1);
    if (wsb < 0) return (int)wsb;
    if (!device_exists(cfg->device)) return op.e_device;
    s->model = m;
    s->cfg = *cfg;
    s->op = op;
    s->rule = r;
    session_restart(s);
    s->frame_bytes = align_up(packed_bytes(cfg->format, H, W));
    s->ws_bytes = align_up(wsb);
    const int64_t t_bytes = align_up(4ll * FLDR_SHUTTER_MAX_SUB), acc_bytes = op.acc_bytes(H, W, cfg->format);
    const int64_t scratch_bytes = op.scratch_bytes(H, W, cfg->format);
    const int64_t dev_total = (2 + n_sub + r.max_out) * s->frame_bytes + acc_bytes + scratch_bytes + t_bytes + FLDR_SCENE_STATE_BYTES + s->ws_bytes;
    const int64_t host_total = (1 + r.max_out) * s->frame_bytes + t_bytes + ALIGN;
    if (!open_stream_mem(s->sm, cfg->device, dev_total, host_total)) return op.e_device;
    s->slot[0] = s->sm.dev;
    s->slot[1] = s->slot[0] + s->frame_bytes;
    s->sub_dev = s->slot[1] + s->frame_bytes;
    s->out_dev = s->sub_dev + n_sub * s->frame_bytes;
    s->acc = s->out_dev + r.max_out * s->frame_bytes;
    s->scratch = (char*)s->acc + acc_bytes;
    s->t_dev = (float*)((char*)s->scratch + scratch_bytes);
    s->state_dev = (char*)s->t_dev + t_bytes;
    s->ws = (char*)s->state_dev + FLDR_SCENE_STATE_BYTES;
    s->in_host = s->sm.pinned;
    s->out_host = s->in_host + s->frame_bytes;
    s->t_host = (float*)(s->out_host + r.max_out * s->frame_bytes);
    s->scene_host = (fldr_scene_result*)((char*)s->t_host + t_bytes);
    return 0;
}

int session_push(Session* s, const fldr_video_frame* frame, const fldr_video_frame* host_outs, fldr_shutter_info* info, int* n_out,
                 fldr_scene_result* scene) {
    const Integration& op = s->op;
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
        if (!host_outs) return op.e_arg;
        for (int k = 0; k < possible; ++k) CK(check_frame(host_outs[k], fmt, W));
    }
    DeviceGuard guard(s->sm.device);
    if (!guard.ok) return op.e_device;
    const hipStream_t stream = s->sm.stream;
    const int cur = s->prev == 0 ? 1 : 0;                          // the slot not holding the previous frame
    hipError_t e = upload_frame(s->sm, s->slot[cur], s->in_host, s->frame_bytes, *frame, fmt, H, W);
    int rc = e == hipSuccess ? 0 : (int)e;
    const int in_slot[2] = { pair ? s->prev : cur, cur };
    fldr_video_frame in[2] = { packed(s->slot[in_slot[0]], fmt, H, W), packed(s->slot[in_slot[1]], fmt, H, W) };
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
    if (rc) { (void)hipStreamSynchronize(stream); session_restart(s); return rc; }
    // ---- the plan: per window, the weight of frame n - 1, of frame n and of each sub-frame k = 1 .. sub - 1 ----
    struct Step { int64_t j; int w_prev, w_cur; uint8_t w_sub[FLDR_SHUTTER_MAX_SUB]; int points, interp, lone; bool begins, ends, truncated; };
    std::vector<Step> steps;
    bool wanted[FLDR_SHUTTER_MAX_SUB] = { false };
    int64_t j = s->j;
    int open_points = s->open_points, open_interp = s->open_interp;
    int64_t open_scene = s->open_scene;
    int open_lone = s->open_lone;
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
        // one point in all, an input frame's samples: the slot that frame lies in (remembered while the window stays open)
        if (open_points + st.points != 1 || open_interp + st.interp != 0) open_lone = -1;
        else if (st.points == 1) open_lone = st.w_prev ? in_slot[0] : in_slot[1];
        st.lone = open_lone;
        open_points += st.points;
        open_interp += st.interp;
        st.points = open_points;
        st.interp = open_interp;
        steps.push_back(st);
        if (!st.ends) break;
        open_points = open_interp = 0;
        open_lone = -1;
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
        fldr_video_frame frames[FLDR_SHUTTER_LAUNCH_FRAMES];
        int32_t weights[FLDR_SHUTTER_LAUNCH_FRAMES];
        int nf = 0;
        if (st.w_prev) { frames[nf] = in[0]; weights[nf++] = st.w_prev; }
        for (int k = 1; k < sub; ++k)
            if (st.w_sub[k]) { frames[nf] = packed(s->sub_dev + slot_of[k] * s->frame_bytes, fmt, H, W); weights[nf++] = st.w_sub[k]; }
        if (st.w_cur) { frames[nf] = in[1]; weights[nf++] = st.w_cur; }
        uint8_t* const out_base = s->out_dev + count * s->frame_bytes;
        const fldr_video_frame out = packed(out_base, fmt, H, W);
        if (op.lone_input_unchanged && st.ends && st.lone >= 0) {
            rc = session_copy_frame(s, s->slot[st.lone], out_base);
        } else if (st.begins && st.ends) {
            rc = op.mix(op.ctx, H, W, fmt, frames, weights, nf, out, s->scratch, stream);     // begins with a point of this push: nf >= 1
        } else {
            if (nf) rc = op.accumulate(op.ctx, H, W, fmt, frames, weights, nf, st.begins, s->acc, s->scratch, stream);
            if (!rc && st.ends) rc = op.resolve(op.ctx, H, W, fmt, s->acc, st.points, out, s->scratch, stream);
        }
        if (st.ends) {
            if (info) { fldr_shutter_info i = { st.j, st.points, st.interp, st.truncated ? 1 : 0, 0 }; info[count] = i; }
            ++count;
        }
    }
    rc = session_deliver(s, rc, count, host_outs);
    if (rc) { session_restart(s); return rc; }     // the held frame and the accumulator are not to be trusted: as after a reset
    if (pair && c.scene == 1 && scene) *scene = *s->scene_host;
    *n_out = count;
    s->j = j;
    s->open_points = open_points; s->open_interp = open_interp; s->open_scene = open_scene; s->open_lone = open_lone;
    if (cut) s->cuts += 1;
    s->n += 1;
    s->prev = cur;
    return 0;
}

int session_flush(Session* s, const fldr_video_frame* host_outs, fldr_shutter_info* info, int* n_out) {
    const Integration& op = s->op;
    *n_out = 0;
    if (s->open_points == 0) return 0;
    if (!host_outs) return op.e_arg;
    const fldr_shutter_config& c = s->cfg;
    CK(check_frame(host_outs[0], c.format, c.W));
    DeviceGuard guard(s->sm.device);
    if (!guard.ok) return op.e_device;
    int rc;
    if (op.lone_input_unchanged && s->open_points == 1 && s->open_lone >= 0) rc = session_copy_frame(s, s->slot[s->open_lone], s->out_dev);
    else rc = op.resolve(op.ctx, c.H, c.W, c.format, s->acc, s->open_points, packed(s->out_dev, c.format, c.H, c.W), s->scratch, s->sm.stream);
    rc = session_deliver(s, rc, 1, host_outs);
    if (rc) { session_restart(s); return rc; }
    if (info) { fldr_shutter_info i = { s->j, s->open_points, s->open_interp, 1, 0 }; info[0] = i; }
    s->j += 1;
    s->open_points = s->open_interp = 0;
    s->open_lone = -1;
    *n_out = 1;
    return 0;
}

}  // namespace
