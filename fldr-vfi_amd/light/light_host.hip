// libfldr_light.so, host side: the curve object and its tables, validation, accumulate / resolve / mix through the video library's
// converters (../video/video_kernels.hip is compiled into this library as shared text, the way frame_host.h is), fldr_light_forward on
// the planar frames fldr_video_forward leaves in its workspace, and the converter — the planner and session of
// ../shutter/session_host.h handed this library's three integration calls, with the checks of sources, blocks and the forward's
// refusals that header shares with libfldr_shutter.so.  The only fldr_* functions called are those of fldr_shutter.h,
// fldr_rate.h, fldr_video.h and fldr_model.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "../shutter/session_host.h"
#include "../video/frame_host.h"
#include "../video/video_internal.h"
#include "light_internal.h"

using namespace fldr_light_impl;
using namespace fldr_video_impl;

struct fldr_light_curve {
    int transfer, depth, device;       // depth: 8 or 10
    uint32_t* dev;                     // lin[codes], mid[codes]
    uint32_t lin[MAX_CODES];
};

namespace {

constexpr uint32_t S = FLDR_LIGHT_SCALE;

// ---- the curves, double precision --------------------------------------------------------------------------------------------------------
double hlg_unscaled(double v) {
    const double a = 0.17883277, b = 1.0 - 4.0 * a, c = 0.5 - a * std::log(4.0 * a);
    return v <= 0.5 ? v * v / 3.0 : (std::exp((v - c) / a) + b) / 12.0;
}

double light_of(int transfer, double v) {
    switch (transfer) {
    case FLDR_LIGHT_GAMMA24: return std::pow(v, 2.4);
    case FLDR_LIGHT_PQ: {
        const double m1 = 2610.0 / 16384.0, m2 = 2523.0 / 4096.0 * 128.0, c1 = 3424.0 / 4096.0, c2 = 2413.0 / 4096.0 * 32.0, c3 = 2392.0 / 4096.0 * 32.0;
        const double e = std::pow(v, 1.0 / m2), num = e - c1 > 0.0 ? e - c1 : 0.0;
        return std::pow(num / (c2 - c3 * e), 1.0 / m1);
    }
    default: return hlg_unscaled(v) / hlg_unscaled(1.0);
    }
}

int depth_of(int depth) { return depth == 0 ? 8 : depth; }

void builtin_table(int transfer, int depth, uint32_t* lin) {
    const int n = 1 << depth;
    lin[0] = 0;
    for (int c = 1; c < n; ++c) {
        const double x = std::floor(light_of(transfer, (double)c / (double)(n - 1)) * (double)S + 0.5);
        const uint32_t v = x <= 0.0 ? 0u : x >= (double)S ? S : (uint32_t)x;
        lin[c] = v > lin[c - 1] ? v : lin[c - 1] + 1;
    }
}

// ---- what one size and format means to the kernels -----------------------------------------------------------------------------------------
struct Plan {
    int H, W;
    fldr_video_format fmt;
    bool deep;
    int64_t count;                     // 3 H W samples of a planar frame
    int64_t frame;                     // its bytes
    int64_t pair_off, out_off, acc_off, total;     // inside scratch
};

int plan_of(int H, int W, const fldr_video_format* fmt, Plan& p) {
    if (!fmt || H < 1 || W < 1) return FLDR_LIGHT_E_ARG;
    CK(check_format(*fmt));
    if (3ll * H * W > 0x7fffffffll) return FLDR_LIGHT_E_ARG;            // the kernels count 16-byte groups in 32 bits
    p.H = H; p.W = W; p.fmt = *fmt;
    p.deep = deep(*fmt);
    p.count = 3ll * H * W;
    p.frame = p.count * (p.deep ? 2 : 1);
    p.pair_off = 0;
    p.out_off = align_up(2 * p.frame);
    p.acc_off = p.out_off + align_up(p.frame);
    p.total = p.acc_off + align_up(4 * p.count);
    return 0;
}

// the curve is looked at last of the host-only checks: every other defect of a call is reported whatever the curve
int check_curve(const fldr_light_curve* c, const fldr_video_format& fmt) {
    if (!c) return FLDR_LIGHT_E_ARG;
    return c->depth == (deep(fmt) ? 10 : 8) ? 0 : FLDR_LIGHT_E_CURVE;
}

Tables tables_of(const fldr_light_curve* c) {
    Tables t = { c->dev, c->dev + (1 << c->depth) };
    return t;
}

const YuvCoeffs& coeffs(const fldr_video_format& f) { return deep(f) ? YUV_COEFFS_10[f.matrix][f.range] : YUV_COEFFS[f.matrix][f.range]; }

int to_planar(const Plan& p, const fldr_video_frame in[2], void* pair, hipStream_t s) {
    return yuv420_to_planar_pair(in, p.fmt, coeffs(p.fmt), pair, p.H, p.W, s);
}

int from_planar(const Plan& p, const void* planar, const fldr_video_frame& out, hipStream_t s) {
    return planar_to_yuv420(planar, out, p.fmt, coeffs(p.fmt), p.H, p.W, s);
}

bool aligned16(const Sources& s) {
    uintptr_t bits = 0;
    for (int k = 0; k < s.n; ++k) bits |= (uintptr_t)s.codes[k];
    return (bits & 15) == 0;
}

// validated arguments -> launches.  Frames go through the planar pair inside scratch two at a time.
int enqueue_accumulate(const Plan& p, const fldr_light_curve* c, const fldr_video_frame* frames, const int32_t* weights, int n, bool first,
                       void* acc, void* scratch, hipStream_t s) {
    uint8_t* pair = (uint8_t*)scratch + p.pair_off;
    Sources src;
    for (int k0 = 0; k0 < n; k0 += 2) {
        const int m = n - k0 < 2 ? 1 : 2;
        const fldr_video_frame in[2] = { frames[k0], frames[k0 + m - 1] };
        CK(to_planar(p, in, pair, s));
        memset(&src, 0, sizeof(src));
        for (int u = 0; u < m; ++u) { src.codes[u] = pair + u * p.frame; src.weight[u] = (uint32_t)weights[k0 + u]; }
        src.n = m;
        CK(launch_accumulate(p.deep, p.count, tables_of(c), src, first && k0 == 0, (uint32_t*)acc, aligned16(src), s));
    }
    return 0;
}

int enqueue_resolve(const Plan& p, const fldr_light_curve* c, const void* acc, int total, const fldr_video_frame& out, void* scratch,
                    hipStream_t s) {
    void* planar = (uint8_t*)scratch + p.out_off;
    CK(launch_resolve(p.deep, p.count, tables_of(c), (const uint32_t*)acc, (uint32_t)total, planar, s));
    return from_planar(p, planar, out, s);
}

int enqueue_mix(const Plan& p, const fldr_light_curve* c, const fldr_video_frame* frames, const int32_t* weights, int n,
                const fldr_video_frame& out, void* scratch, hipStream_t s) {
    int total = 0;
    for (int k = 0; k < n; ++k) total += weights[k];
    if (n > 2) {
        void* acc = (uint8_t*)scratch + p.acc_off;
        CK(enqueue_accumulate(p, c, frames, weights, n, true, acc, scratch, s));
        return enqueue_resolve(p, c, acc, total, out, scratch, s);
    }
    uint8_t* pair = (uint8_t*)scratch + p.pair_off;
    void* planar = (uint8_t*)scratch + p.out_off;
    const fldr_video_frame in[2] = { frames[0], frames[n - 1] };
    CK(to_planar(p, in, pair, s));
    Sources src;
    memset(&src, 0, sizeof(src));
    for (int u = 0; u < n; ++u) { src.codes[u] = pair + u * p.frame; src.weight[u] = (uint32_t)weights[u]; }
    src.n = n;
    CK(launch_mix(p.deep, p.count, tables_of(c), src, (uint32_t)total, planar, aligned16(src), s));
    return from_planar(p, planar, out, s);
}

}  // namespace

extern "C" FLDR_LIGHT_API int fldr_light_version(void) { return FLDR_LIGHT_VERSION; }

extern "C" FLDR_LIGHT_API const char* fldr_light_error_string(int code) {
    switch (code) {
    case 0: return "success";
    case FLDR_LIGHT_E_ARG: return "fldr_light: bad argument";
    case FLDR_LIGHT_E_CURVE: return "fldr_light: the curve's depth is not the format's";
    case FLDR_LIGHT_E_TABLE: return "fldr_light: table not strictly increasing or above 2^24 - 1";
    case FLDR_LIGHT_E_ACC: return "fldr_light: accumulator or scratch missing or misaligned";
    case FLDR_LIGHT_E_WEIGHT: return "fldr_light: a weight or a total outside its range";
    case FLDR_LIGHT_E_RATIO: return "fldr_light: rate or shutter terms outside what the converter takes";
    case FLDR_LIGHT_E_DEVICE: return "fldr_light: no such device or out of memory";
    case FLDR_LIGHT_E_FORMAT: return "fldr_light: in_format and out_format differ";
    default: return code > -400 ? fldr_shutter_error_string(code) : "fldr_light: unknown error";
    }
}

extern "C" FLDR_LIGHT_API int fldr_light_sizeof(int which) { return which == 0 ? (int)sizeof(fldr_light_config) : FLDR_LIGHT_E_ARG; }

// ---- the curve ----------------------------------------------------------------------------------------------------------------------------
extern "C" FLDR_LIGHT_API int fldr_light_table(int transfer, int depth, uint32_t* lin) {
    depth = depth_of(depth);
    if (!lin || (depth != 8 && depth != 10) || transfer < FLDR_LIGHT_GAMMA24 || transfer > FLDR_LIGHT_HLG) return FLDR_LIGHT_E_ARG;
    builtin_table(transfer, depth, lin);
    return 0;
}

extern "C" FLDR_LIGHT_API int fldr_light_curve_create(int transfer, int depth, const uint32_t* table, int device, fldr_light_curve** out) {
    if (!out) return FLDR_LIGHT_E_ARG;
    *out = nullptr;
    depth = depth_of(depth);
    if ((depth != 8 && depth != 10) || transfer < FLDR_LIGHT_GAMMA24 || transfer > FLDR_LIGHT_TABLE || device < 0) return FLDR_LIGHT_E_ARG;
    const int n = 1 << depth;
    fldr_light_curve* c = new (std::nothrow) fldr_light_curve();
    if (!c) return FLDR_LIGHT_E_DEVICE;
    c->transfer = transfer; c->depth = depth; c->device = device; c->dev = nullptr;
    if (transfer == FLDR_LIGHT_TABLE) {
        if (!table) { delete c; return FLDR_LIGHT_E_ARG; }
        bool ok = table[n - 1] <= S;
        for (int i = 1; i < n && ok; ++i) ok = table[i] > table[i - 1];
        if (!ok) { delete c; return FLDR_LIGHT_E_TABLE; }
        memcpy(c->lin, table, sizeof(uint32_t) * n);
    } else {
        builtin_table(transfer, depth, c->lin);
    }
    std::vector<uint32_t> both((size_t)2 * n);
    memcpy(both.data(), c->lin, sizeof(uint32_t) * n);
    both[n] = 0;
    for (int i = 1; i < n; ++i) both[n + i] = c->lin[i - 1] + c->lin[i];
    if (!device_exists(device)) { delete c; return FLDR_LIGHT_E_DEVICE; }
    DeviceGuard guard(device);
    if (!guard.ok || hipMalloc((void**)&c->dev, both.size() * sizeof(uint32_t)) != hipSuccess) { (void)hipGetLastError(); delete c; return FLDR_LIGHT_E_DEVICE; }
    const hipError_t e = hipMemcpy(c->dev, both.data(), both.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(c->dev); delete c; return (int)e; }
    *out = c;
    return 0;
}

extern "C" FLDR_LIGHT_API void fldr_light_curve_destroy(fldr_light_curve* c) {
    if (!c) return;
    { DeviceGuard guard(c->device); (void)hipFree(c->dev); (void)hipGetLastError(); }
    delete c;
}

// ---- the integration kernels ------------------------------------------------------------------------------------------------------------------
extern "C" FLDR_LIGHT_API int64_t fldr_light_acc_bytes(int H, int W) {
    if (H < 1 || W < 1 || 3ll * H * W > 0x7fffffffll) return FLDR_LIGHT_E_ARG;
    return align_up(12ll * H * W);
}

extern "C" FLDR_LIGHT_API int64_t fldr_light_scratch_bytes(int H, int W, const fldr_video_format* fmt) {
    Plan p;
    const int rc = plan_of(H, W, fmt, p);
    return rc ? rc : p.total;
}

extern "C" FLDR_LIGHT_API int fldr_light_accumulate(int H, int W, const fldr_video_format* fmt, const fldr_light_curve* curve,
                                                    const fldr_video_frame* frames, const int32_t* weights, int n, int first, void* acc,
                                                    void* scratch, void* stream) {
    Plan p;
    CK(plan_of(H, W, fmt, p));
    CK(check_sources(p.fmt, W, frames, weights, n, FLDR_LIGHT_E_ARG, FLDR_LIGHT_E_WEIGHT, FLDR_LIGHT_MAX_TOTAL));
    CK(check_aligned(acc, FLDR_LIGHT_E_ACC));
    CK(check_aligned(scratch, FLDR_LIGHT_E_ACC));
    CK(check_curve(curve, p.fmt));
    return enqueue_accumulate(p, curve, frames, weights, n, first != 0, acc, scratch, (hipStream_t)stream);
}

extern "C" FLDR_LIGHT_API int fldr_light_resolve(int H, int W, const fldr_video_format* fmt, const fldr_light_curve* curve, const void* acc,
                                                 int total, const fldr_video_frame* out, void* scratch, void* stream) {
    Plan p;
    CK(plan_of(H, W, fmt, p));
    if (!out) return FLDR_LIGHT_E_ARG;
    CK(check_frame(*out, p.fmt, W));
    if (total < 1 || total > FLDR_LIGHT_MAX_TOTAL) return FLDR_LIGHT_E_WEIGHT;
    CK(check_aligned(acc, FLDR_LIGHT_E_ACC));
    CK(check_aligned(scratch, FLDR_LIGHT_E_ACC));
    CK(check_curve(curve, p.fmt));
    return enqueue_resolve(p, curve, acc, total, *out, scratch, (hipStream_t)stream);
}

extern "C" FLDR_LIGHT_API int fldr_light_mix(int H, int W, const fldr_video_format* fmt, const fldr_light_curve* curve,
                                             const fldr_video_frame* frames, const int32_t* weights, int n, const fldr_video_frame* out,
                                             void* scratch, void* stream) {
    Plan p;
    CK(plan_of(H, W, fmt, p));
    if (n > MAX_FRAMES || !out) return FLDR_LIGHT_E_ARG;
    CK(check_sources(p.fmt, W, frames, weights, n, FLDR_LIGHT_E_ARG, FLDR_LIGHT_E_WEIGHT, FLDR_LIGHT_MAX_TOTAL));
    CK(check_frame(*out, p.fmt, W));
    CK(check_aligned(scratch, FLDR_LIGHT_E_ACC));
    CK(check_curve(curve, p.fmt));
    return enqueue_mix(p, curve, frames, weights, n, *out, scratch, (hipStream_t)stream);
}

// ---- one pair ---------------------------------------------------------------------------------------------------------------------------
namespace {

int64_t largest_scratch(int H, int W) {
    fldr_video_format f;
    memset(&f, 0, sizeof(f));
    f.depth = 10;
    Plan p;
    const int rc = plan_of(H, W, &f, p);
    return rc ? rc : p.total;
}

}  // namespace

extern "C" FLDR_LIGHT_API int64_t fldr_light_workspace_bytes(const fldr_model* m, int H, int W, int n_t) {
    const int64_t vb = fldr_video_workspace_bytes(m, H, W, n_t);
    if (vb < 0) return vb;
    const int64_t sb = largest_scratch(H, W);
    return sb < 0 ? sb : align_up(vb) + align_up(12ll * H * W) + sb;
}

extern "C" FLDR_LIGHT_API int fldr_light_forward(const fldr_model* m, const fldr_video_io* io, const fldr_light_curve* curve, int w0, int w1,
                                                 const int32_t* w, void* ws, int64_t ws_bytes, void* stream) {
    // everything fldr_video_forward and the mix would refuse is refused here, before anything is enqueued
    int total;
    CK(forward_preamble(io, w0, w1, w, FLDR_LIGHT_E_ARG, FLDR_LIGHT_E_FORMAT, FLDR_LIGHT_E_WEIGHT, FLDR_LIGHT_MAX_TOTAL, &total));
    const fldr_video_format& fmt = io->in_format;
    const int H = io->H, W = io->W, n_t = io->n_t;
    Plan p;
    CK(plan_of(H, W, &fmt, p));
    CK(check_curve(curve, fmt));
    const int64_t vb = fldr_video_workspace_bytes(m, H, W, n_t);
    if (vb < 0) return (int)vb;
    const int64_t mb = fldr_model_workspace_bytes(m, H, W, n_t);
    if (mb < 0) return (int)mb;
    const int64_t scratch_off = align_up(vb) + align_up(12ll * H * W), sb = largest_scratch(H, W);
    if (!ws || ((uintptr_t)ws & (ALIGN - 1)) || ws_bytes < scratch_off + sb) return FLDR_VIDEO_E_WORKSPACE;
    uint8_t* scratch = (uint8_t*)ws + scratch_off;
    // the n_t frames fldr_video_forward must write are not wanted: all of them land, one after the other, in the unused pair of scratch
    const fldr_video_frame unwanted = packed(scratch + p.pair_off, fmt, H, W);
    std::vector<fldr_video_frame> subs((size_t)n_t, unwanted);
    fldr_video_io inner = *io;
    inner.out = subs.data();
    CK(fldr_video_forward(m, &inner, ws, align_up(vb), stream));
    // where fldr_video_forward left the points (fldr_video.h): the planar pair behind the model's part, the n_t planar outputs behind it
    const uint8_t* pair = (const uint8_t*)ws + align_up(mb);
    const uint8_t* outs = pair + align_up(2 * p.frame);
    const int64_t stride = align_up(p.frame);
    Sources src;
    memset(&src, 0, sizeof(src));
    int n = 0;
    if (w0) { src.codes[n] = pair; src.weight[n++] = (uint32_t)w0; }
    if (w1) { src.codes[n] = pair + p.frame; src.weight[n++] = (uint32_t)w1; }
    for (int k = 0; k < n_t; ++k) { src.codes[n] = outs + k * stride; src.weight[n++] = (uint32_t)w[k]; }
    src.n = n;
    void* planar = scratch + p.out_off;
    CK(launch_mix(p.deep, p.count, tables_of(curve), src, (uint32_t)total, planar, aligned16(src), (hipStream_t)stream));
    return from_planar(p, planar, io->out[0], (hipStream_t)stream);
}

// ---- the converter ------------------------------------------------------------------------------------------------------------------------
namespace {

int op_check(void* ctx, int H, int W, const fldr_video_format& fmt) {
    Plan p;
    CK(plan_of(H, W, &fmt, p));
    return check_curve((const fldr_light_curve*)ctx, fmt);
}

int64_t op_acc_bytes(int H, int W, const fldr_video_format&) { return align_up(12ll * H * W); }

int64_t op_scratch_bytes(int H, int W, const fldr_video_format& fmt) {
    Plan p;
    plan_of(H, W, &fmt, p);
    return p.total;
}

int op_accumulate(void* ctx, int H, int W, const fldr_video_format& fmt, const fldr_video_frame* frames, const int32_t* weights, int n,
                  bool first, void* acc, void* scratch, hipStream_t s) {
    Plan p;
    plan_of(H, W, &fmt, p);
    return enqueue_accumulate(p, (const fldr_light_curve*)ctx, frames, weights, n, first, acc, scratch, s);
}

int op_resolve(void* ctx, int H, int W, const fldr_video_format& fmt, const void* acc, int total, const fldr_video_frame& out, void* scratch,
               hipStream_t s) {
    Plan p;
    plan_of(H, W, &fmt, p);
    return enqueue_resolve(p, (const fldr_light_curve*)ctx, acc, total, out, scratch, s);
}

int op_mix(void* ctx, int H, int W, const fldr_video_format& fmt, const fldr_video_frame* frames, const int32_t* weights, int n,
           const fldr_video_frame& out, void* scratch, hipStream_t s) {
    Plan p;
    plan_of(H, W, &fmt, p);
    return enqueue_mix(p, (const fldr_light_curve*)ctx, frames, weights, n, out, scratch, s);
}

}  // namespace

struct fldr_light { Session s; };

extern "C" FLDR_LIGHT_API int fldr_light_create(const fldr_model* m, const fldr_light_config* cfg, fldr_light** out) {
    if (!cfg || !out) return FLDR_LIGHT_E_ARG;
    *out = nullptr;
    const Integration linear_mean = { (void*)cfg->curve, FLDR_LIGHT_E_ARG, FLDR_LIGHT_E_RATIO, FLDR_LIGHT_E_DEVICE, FLDR_LIGHT_MAX_TOTAL, true,
                                      op_check, op_acc_bytes, op_scratch_bytes, op_accumulate, op_resolve, op_mix };
    fldr_light* h = new (std::nothrow) fldr_light();
    if (!h) return FLDR_LIGHT_E_DEVICE;
    int rc = session_open(&h->s, m, &cfg->shutter, linear_mean);
    if (!rc && cfg->curve->device != cfg->shutter.device) { close_stream_mem(h->s.sm); rc = FLDR_LIGHT_E_ARG; }
    if (rc) { delete h; return rc; }
    *out = h;
    return 0;
}

extern "C" FLDR_LIGHT_API int fldr_light_max_out(const fldr_light* h) { return h ? h->s.rule.max_out : FLDR_LIGHT_E_ARG; }

extern "C" FLDR_LIGHT_API int fldr_light_push(fldr_light* h, const fldr_video_frame* frame, const fldr_video_frame* host_outs,
                                              fldr_shutter_info* info, int* n_out, fldr_scene_result* scene) {
    if (!h || !frame || !n_out) return FLDR_LIGHT_E_ARG;
    return session_push(&h->s, frame, host_outs, info, n_out, scene);
}

extern "C" FLDR_LIGHT_API int fldr_light_flush(fldr_light* h, const fldr_video_frame* host_outs, fldr_shutter_info* info, int* n_out) {
    if (!h || !n_out) return FLDR_LIGHT_E_ARG;
    return session_flush(&h->s, host_outs, info, n_out);
}

extern "C" FLDR_LIGHT_API int fldr_light_reset(fldr_light* h) {
    if (!h) return FLDR_LIGHT_E_ARG;
    session_restart(&h->s);
    return 0;
}

extern "C" FLDR_LIGHT_API void fldr_light_destroy(fldr_light* h) {
    if (h) { close_stream_mem(h->s.sm); delete h; }
}
