// libfldr_scale.so, host side: the tables (scale_taps.h), the map, validation, fldr_scale_frame, fldr_scale_forward (scale -> forward or
// forward -> scale, by the map's placement) and the stream (host frames at the in size and rate in, host frames at the out size and rate
// out).  The video API's rules for formats and frames, the padded frames, the extents of the overlap test and the device / stream /
// pinned block of a stream object come from ../video/frame_host.h; the configuration rules and the schedule of the rate converter from
// ../rate/rate_plan.h, which includes it; the order in which several frames are checked from ../rate/tile_measure_host.h.  The only
// fldr_* functions called are those of fldr_rate.h, fldr_video.h and fldr_model.h.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <vector>

#include "../rate/rate_plan.h"
#include "../rate/tile_measure_host.h"
#include "scale_internal.h"
#include "scale_taps.h"

using namespace fldr_scale_impl;

namespace {

bool same_format(const fldr_video_format& a, const fldr_video_format& b) {
    return a.layout == b.layout && a.matrix == b.matrix && a.range == b.range && deep(a) == deep(b);
}

bool map_ok(const fldr_scale_map* m) { return m && m->live == FLDR_SCALE_MAP_LIVE && m->tables; }

int resolve_where(int where, int iH, int iW, int oH, int oW) {
    if (where != FLDR_SCALE_AUTO) return where;
    return (int64_t)oH * oW < (int64_t)iH * iW ? FLDR_SCALE_BEFORE : FLDR_SCALE_AFTER;
}

// the size, filter and placement words every entry shares (FLDR_RATE_E_ARG), then the tap limit of both axes
int check_scale_words(int iH, int iW, int oH, int oW, int filter, int where, const int32_t* reserved, int n_reserved, bool limits) {
    if (!scale_size_ok(iH) || !scale_size_ok(iW) || !scale_size_ok(oH) || !scale_size_ok(oW)) return FLDR_RATE_E_ARG;
    if ((unsigned)filter > (unsigned)FLDR_SCALE_LANCZOS3 || (unsigned)where > (unsigned)FLDR_SCALE_AUTO) return FLDR_RATE_E_ARG;
    for (int i = 0; i < n_reserved; ++i) if (reserved[i]) return FLDR_RATE_E_ARG;
    if (limits && (scale_taps_count(iW, oW, filter) < 0 || scale_taps_count(iH, oH, filter) < 0)) return FLDR_RATE_E_ARG;
    return 0;
}

int check_map_config(const fldr_scale_map_config& c) {
    CK(check_scale_words(c.in_H, c.in_W, c.out_H, c.out_W, c.filter, c.where, c.reserved, 3, false));
    if (c.device < 0 || (unsigned)c.read > (unsigned)FLDR_SCALE_READ_STAGED) return FLDR_RATE_E_ARG;
    CK(check_format(c.format));
    return check_scale_words(c.in_H, c.in_W, c.out_H, c.out_W, c.filter, c.where, c.reserved, 3, true);
}

// the most source rows a tile of th output rows needs: what the kernel forms from the first and last left_y of the tile
int max_span(const int32_t* left_y, int out_rows, int in_rows, int ny, int th) {
    int worst = 0;
    for (int y0 = 0; y0 < out_rows; y0 += th) {
        const int y1 = y0 + th < out_rows ? y0 + th : out_rows;
        const int lo = std::min(std::max(left_y[y0], 0), in_rows - 1), hi = std::min(std::max(left_y[y1 - 1] + ny - 1, 0), in_rows - 1);
        worst = std::max(worst, hi - lo + 1);
    }
    return worst;
}

// the most source samples of a row a tile of tw output samples reads: what the staged kernel forms from the first and last left_x of the tile
int max_stage_span(const int32_t* left_x, int out_w, int in_cols, int nx, int tw, int cshift) {
    int worst = 0;
    for (int x0 = 0; x0 < out_w; x0 += tw) {
        const int x1 = x0 + tw < out_w ? x0 + tw : out_w;
        const int lo = std::min(std::max(left_x[x0 >> cshift], 0), in_cols - 1);
        const int hi = std::min(std::max(left_x[(x1 - 1) >> cshift] + nx - 1, 0), in_cols - 1);
        worst = std::max(worst, (hi - lo + 1) << cshift);
    }
    return worst;
}

struct HostTable { std::vector<int32_t> left; std::vector<int16_t> coef; };

int build_table(int in, int out, int filter, int kind, int n, HostTable& t) {
    const int outputs = scale_outputs(out, kind);
    t.left.resize((size_t)outputs);
    t.coef.resize((size_t)outputs * n);
    return scale_taps(in, out, filter, kind, t.left.data(), t.coef.data());
}

// the launch arguments of a checked call
void fill_args(const fldr_scale_map& m, const fldr_video_frame& in, const fldr_video_frame& out, ScaleArgs& a) {
    const fldr_scale_map_config& c = m.cfg;
    memset(&a, 0, sizeof(a));
    a.planes = planes_of(c.format.layout);
    a.nx = m.taps_x; a.ny = m.taps_y;
    a.stage_at = m.stage_at / 2;
    const uint8_t* tb = (const uint8_t*)m.tables;
    uint32_t first = 0;
    for (int p = 0; p < a.planes; ++p) {
        ScalePlane& q = a.pl[p];
        const int j = p ? 1 : 0;
        q.src = (const uint8_t*)in.plane[p]; q.pitch_src = in.pitch[p];
        q.dst = (uint8_t*)out.plane[p]; q.pitch_dst = out.pitch[p];
        q.left_x = (const int32_t*)(tb + m.offset[4 * j]); q.coef_x = (const int16_t*)(tb + m.offset[4 * j + 1]);
        q.left_y = (const int32_t*)(tb + m.offset[4 * j + 2]); q.coef_y = (const int16_t*)(tb + m.offset[4 * j + 3]);
        q.cshift = p && c.format.layout == FLDR_VIDEO_NV12 ? 1 : 0;
        q.in_cols = p ? (c.in_W + 1) / 2 : c.in_W;
        q.in_rows = rows_of(p, c.in_H);
        q.out_w = (p ? (c.out_W + 1) / 2 : c.out_W) << q.cshift;
        q.out_rows = rows_of(p, c.out_H);
        q.tile_w = m.tile_w[j]; q.tile_h = m.tile_h[j];
        q.stage_span = m.stage_span[j];
        q.vec = (((uintptr_t)q.dst | (uintptr_t)q.pitch_dst) & 15) == 0 ? 1 : 0;
        q.tiles_x = (uint32_t)((q.out_w + q.tile_w - 1) / q.tile_w);
        q.first = first;
        first += q.tiles_x * (uint32_t)((q.out_rows + q.tile_h - 1) / q.tile_h);
    }
    a.total = first;
}

// any plane of `out` (oH x oW) shares a byte with any plane of `in` (iH x iW)
bool overlaps2(const fldr_video_frame& out, int oH, int oW, const fldr_video_frame& in, int iH, int iW, const fldr_video_format& fmt) {
    for (int p = 0; p < planes_of(fmt.layout); ++p)
        for (int q = 0; q < planes_of(fmt.layout); ++q) {
            uintptr_t a0, a1, b0, b1;
            extent(out, fmt, p, oH, oW, a0, a1);
            extent(in, fmt, q, iH, iW, b0, b1);
            if (a0 < b1 && b0 < a1) return true;
        }
    return false;
}

int check_scale_frame(const fldr_scale_map* map, const fldr_video_frame* in, const fldr_video_frame* out) {
    if (!map_ok(map)) return FLDR_RATE_E_STATE;
    if (!in || !out) return FLDR_RATE_E_ARG;
    const fldr_scale_map_config& c = map->cfg;
    CK(check_frames(&in, 1, c.format, c.in_W));
    CK(check_frames(&out, 1, c.format, c.out_W));
    if (overlaps2(*out, c.out_H, c.out_W, *in, c.in_H, c.in_W, c.format)) return FLDR_RATE_E_ARG;
    return 0;
}

int enqueue_scale(const fldr_scale_map& m, const fldr_video_frame& in, const fldr_video_frame& out, hipStream_t stream) {
    ScaleArgs a;
    fill_args(m, in, out, a);
    return scale(a, luma_mode(deep(m.cfg.format), m.cfg.format.layout), m.lds_bytes, stream);
}

// ---- the workspace of a forward: the rate forward's at the size it runs at, then the temporaries at that size ---------------------------
struct ForwardWs { int fH, fW, temps; int64_t rate_bytes, temp0, temp_bytes, total; };

int64_t plan_ws(const fldr_model* m, const fldr_scale_map* map, int n_t, ForwardWs& ws) {
    if (!map_ok(map)) return FLDR_RATE_E_STATE;
    if (n_t < 1 || n_t > FLDR_RATE_MAX_OUT) return FLDR_RATE_E_ARG;
    const bool before = map->where == FLDR_SCALE_BEFORE;
    ws.fH = before ? map->cfg.out_H : map->cfg.in_H;
    ws.fW = before ? map->cfg.out_W : map->cfg.in_W;
    ws.temps = before ? 2 : n_t;
    const int64_t rb = fldr_rate_workspace_bytes(m, ws.fH, ws.fW, n_t);
    if (rb < 0) return rb;
    ws.rate_bytes = rb;
    ws.temp0 = align_up(rb);
    ws.temp_bytes = align_up(padded_bytes(map->cfg.format, ws.fH, ws.fW));
    ws.total = ws.temp0 + ws.temps * ws.temp_bytes;
    return ws.total;
}

}  // namespace

extern "C" FLDR_SCALE_API int fldr_scale_version(void) { return FLDR_SCALE_VERSION; }

extern "C" FLDR_SCALE_API const char* fldr_scale_error_string(int code) { return fldr_rate_error_string(code); }

extern "C" FLDR_SCALE_API int fldr_scale_sizeof(int which) {
    switch (which) {
    case 0: return (int)sizeof(fldr_scale_map_config);
    case 1: return (int)sizeof(fldr_scale_map);
    case 2: return (int)sizeof(fldr_scale_io);
    case 3: return (int)sizeof(fldr_scale_config);
    default: return FLDR_RATE_E_ARG;
    }
}

extern "C" FLDR_SCALE_API int fldr_scale_taps_count(int luma_in, int luma_out, int filter) { return scale_taps_count(luma_in, luma_out, filter); }

extern "C" FLDR_SCALE_API int fldr_scale_taps(int luma_in, int luma_out, int filter, int kind, int32_t* left, int16_t* coef) {
    return scale_taps(luma_in, luma_out, filter, kind, left, coef);
}

// ---- the map ---------------------------------------------------------------------------------------------------------------------------
extern "C" FLDR_SCALE_API int fldr_scale_map_create(const fldr_scale_map_config* cfg, fldr_scale_map* map) {
    if (map) memset(map, 0, sizeof(*map));
    if (!cfg || !map) return FLDR_RATE_E_ARG;
    CK(check_map_config(*cfg));
    const fldr_scale_map_config& c = *cfg;
    const int nx = scale_taps_count(c.in_W, c.out_W, c.filter), ny = scale_taps_count(c.in_H, c.out_H, c.filter);
    HostTable t[4];                                                    // luma x, luma y, chroma x, chroma y
    CK(build_table(c.in_W, c.out_W, c.filter, FLDR_SCALE_LUMA, nx, t[0]));
    CK(build_table(c.in_H, c.out_H, c.filter, FLDR_SCALE_LUMA, ny, t[1]));
    CK(build_table(c.in_W, c.out_W, c.filter, FLDR_SCALE_CHROMA_H, nx, t[2]));
    CK(build_table(c.in_H, c.out_H, c.filter, FLDR_SCALE_CHROMA_V, ny, t[3]));
    fldr_scale_map m;
    memset(&m, 0, sizeof(m));
    m.cfg = c;
    m.where = resolve_where(c.where, c.in_H, c.in_W, c.out_H, c.out_W);
    m.taps_x = nx; m.taps_y = ny;
    const int tw = TILE_GROUPS * (deep(c.format) ? 8 : 16);
    // the staged read: a chunk of source rows of the widest tile's source samples, as 16-bit words, for both plane kinds
    const int stage_rows = STAGE_ROWS_BYTE * (deep(c.format) ? 2 : 1);
    int span[2], stage_bytes = 0;
    for (int j = 0; j < 2; ++j) {
        const int cshift = j && c.format.layout == FLDR_VIDEO_NV12 ? 1 : 0;
        const int out_w = (j ? (c.out_W + 1) / 2 : c.out_W) << cshift;
        span[j] = max_stage_span(t[2 * j].left.data(), out_w, j ? (c.in_W + 1) / 2 : c.in_W, nx, tw, cshift);
        stage_bytes = std::max(stage_bytes, stage_rows * span[j] * 2);
    }
    const bool fits = stage_bytes <= STAGE_LIMIT;
    if (c.read == FLDR_SCALE_READ_STAGED && !fits) return FLDR_RATE_E_ARG;
    // AUTO, by measurement (DESIGN_LOG.md): staging pays where a source sample is read by many taps and the pass is a large part of the
    // kernel — reductions under the two wide filters; enlargements and bilinear are faster reading directly
    const bool wanted = c.read == FLDR_SCALE_READ_STAGED || (c.read == FLDR_SCALE_READ_AUTO && c.in_W > c.out_W && c.filter != FLDR_SCALE_BILINEAR);
    const bool staged = wanted && fits;
    m.read = staged ? FLDR_SCALE_READ_STAGED : FLDR_SCALE_READ_DIRECT;
    if (!staged) stage_bytes = 0;
    int m_bytes = 0;
    for (int j = 0; j < 2; ++j) {
        const int out_rows = rows_of(j, c.out_H), in_rows = rows_of(j, c.in_H);
        int th = TILE_ROWS_MAX;
        // a tile of one output row needs at most ny <= 64 source rows of tw int16: 32 KB, so the loop ends at or before th = 1
        while (th > 1 && (int64_t)max_span(t[2 * j + 1].left.data(), out_rows, in_rows, ny, th) * tw * 2 > LDS_LIMIT - stage_bytes) th >>= 1;
        m.tile_w[j] = tw; m.tile_h[j] = th;
        m.stage_span[j] = staged ? span[j] : 0;
        m_bytes = std::max(m_bytes, max_span(t[2 * j + 1].left.data(), out_rows, in_rows, ny, th) * tw * 2);
    }
    m.stage_at = staged ? m_bytes : 0;
    m.lds_bytes = m_bytes + stage_bytes;
    int64_t bytes = 0;
    for (int i = 0; i < 4; ++i) {
        m.offset[2 * i] = bytes; bytes += align_up((int64_t)t[i].left.size() * 4);
        m.offset[2 * i + 1] = bytes; bytes += align_up((int64_t)t[i].coef.size() * 2);
    }
    if (!device_exists(c.device)) return FLDR_RATE_E_DEVICE;
    DeviceGuard g(c.device);
    if (!g.ok) return FLDR_RATE_E_DEVICE;
    if (hipMalloc(&m.tables, (size_t)bytes) != hipSuccess) { (void)hipGetLastError(); return FLDR_RATE_E_DEVICE; }
    hipError_t e = hipSuccess;
    for (int i = 0; i < 4 && e == hipSuccess; ++i) {
        e = hipMemcpy((uint8_t*)m.tables + m.offset[2 * i], t[i].left.data(), t[i].left.size() * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy((uint8_t*)m.tables + m.offset[2 * i + 1], t[i].coef.data(), t[i].coef.size() * 2, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { (void)hipFree(m.tables); (void)hipGetLastError(); return (int)e; }
    m.live = FLDR_SCALE_MAP_LIVE;
    *map = m;
    return 0;
}

extern "C" FLDR_SCALE_API void fldr_scale_map_destroy(fldr_scale_map* map) {
    if (!map_ok(map)) return;
    DeviceGuard g(map->cfg.device);
    (void)hipFree(map->tables);
    (void)hipGetLastError();
    memset(map, 0, sizeof(*map));
}

extern "C" FLDR_SCALE_API int fldr_scale_frame(const fldr_scale_map* map, const fldr_video_frame* in, const fldr_video_frame* out, void* stream) {
    CK(check_scale_frame(map, in, out));
    return enqueue_scale(*map, *in, *out, (hipStream_t)stream);
}

// ---- the forward -------------------------------------------------------------------------------------------------------------------------
extern "C" FLDR_SCALE_API int64_t fldr_scale_workspace_bytes(const fldr_model* m, const fldr_scale_map* map, int n_t) {
    ForwardWs ws;
    return plan_ws(m, map, n_t, ws);
}

extern "C" FLDR_SCALE_API int fldr_scale_temp_frame(const fldr_model* m, const fldr_scale_map* map, const fldr_video_format* fmt, int n_t, int k, void* ws,
                                                    fldr_video_frame* frame) {
    if (!fmt || !frame) return FLDR_RATE_E_ARG;
    ForwardWs lay;
    const int64_t total = plan_ws(m, map, n_t, lay);
    if (total < 0) return (int)total;
    if (k < 0 || k >= lay.temps) return FLDR_RATE_E_ARG;
    CK(check_format(*fmt));
    if (!same_format(*fmt, map->cfg.format)) return FLDR_RATE_E_FORMAT;
    if (!ws || ((uintptr_t)ws & (ALIGN - 1))) return FLDR_RATE_E_ARG;
    *frame = padded((uint8_t*)ws + lay.temp0 + k * lay.temp_bytes, *fmt, lay.fH, lay.fW);
    return 0;
}

extern "C" FLDR_SCALE_API int fldr_scale_forward(const fldr_model* m, const fldr_scale_map* map, const fldr_scale_io* io, void* ws, int64_t ws_bytes,
                                                 void* stream) {
    if (!io) return FLDR_RATE_E_ARG;
    if (!map_ok(map)) return FLDR_RATE_E_STATE;
    const fldr_video_io& v = io->v;
    const fldr_scale_map_config& c = map->cfg;
    const int n_t = v.n_t;
    if (v.H != c.in_H || v.W != c.in_W || n_t < 1 || n_t > FLDR_RATE_MAX_OUT || !v.t || !v.out || (unsigned)io->scene > 1u) return FLDR_RATE_E_ARG;
    for (int i = 0; i < 4; ++i) if (io->reserved[i]) return FLDR_RATE_E_ARG;
    CK(check_scene_params(io->scene_params));
    CK(check_format(v.in_format));
    CK(check_format(v.out_format));
    if (!same_format(v.in_format, v.out_format) || !same_format(v.in_format, c.format)) return FLDR_RATE_E_FORMAT;
    const fldr_video_format& fmt = c.format;
    const fldr_video_frame* ins[2] = { &v.in[0], &v.in[1] };
    CK(check_frames(ins, 2, fmt, c.in_W));
    const fldr_video_frame* outs[FLDR_RATE_MAX_OUT];
    for (int k = 0; k < n_t; ++k) outs[k] = &v.out[k];
    CK(check_frames(outs, n_t, fmt, c.out_W));
    if (!m) return FLDR_RATE_E_ARG;
    ForwardWs lay;
    const int64_t total = plan_ws(m, map, n_t, lay);
    if (total < 0) return (int)total;
    if (!ws || ((uintptr_t)ws & (ALIGN - 1)) || ws_bytes < total) return FLDR_RATE_E_ARG;
    uint8_t* w = (uint8_t*)ws;
    for (int k = 0; k < n_t; ++k) {
        for (int f = 0; f < 2; ++f) if (overlaps2(v.out[k], c.out_H, c.out_W, v.in[f], c.in_H, c.in_W, fmt)) return FLDR_RATE_E_ARG;
        // an output anywhere inside the workspace would be written by the forward or read as a temporary
        for (int p = 0; p < planes_of(fmt.layout); ++p) {
            uintptr_t lo, hi;
            extent(v.out[k], fmt, p, c.out_H, c.out_W, lo, hi);
            if (lo < (uintptr_t)w + (uintptr_t)total && (uintptr_t)w < hi) return FLDR_RATE_E_ARG;
        }
    }
    // everything has been checked
    const hipStream_t s = (hipStream_t)stream;
    fldr_video_frame temp[FLDR_RATE_MAX_OUT];
    for (int k = 0; k < lay.temps; ++k) temp[k] = padded(w + lay.temp0 + k * lay.temp_bytes, fmt, lay.fH, lay.fW);
    fldr_video_io vio = v;
    vio.H = lay.fH; vio.W = lay.fW;
    vio.in_format = vio.out_format = fmt;
    const bool before = map->where == FLDR_SCALE_BEFORE;
    if (before) {
        for (int f = 0; f < 2; ++f) { CK(enqueue_scale(*map, v.in[f], temp[f], s)); vio.in[f] = temp[f]; }
    } else {
        vio.out = temp;
    }
    if (io->scene) CK(fldr_rate_forward(m, &vio, &io->scene_params, ws, lay.rate_bytes, stream));
    else CK(fldr_video_forward(m, &vio, ws, lay.rate_bytes, stream));
    if (!before) for (int k = 0; k < n_t; ++k) CK(enqueue_scale(*map, temp[k], v.out[k], s));
    return 0;
}

// ---- the stream ------------------------------------------------------------------------------------------------------------------------
struct fldr_scale {
    const fldr_model* model;
    fldr_scale_config cfg;
    RatePlan plan;
    fldr_scale_map map;
    bool before, forwards;
    int fH, fW;                        // the size the slots are kept and the forward runs at
    // device: the uploaded frame (BEFORE: it is scaled into its slot), slot 0, slot 1, max_out forward outputs (at fH x fW), max_out scaled
    //         outputs (AFTER), t, the scene state of pairs without a forward, the workspace
    // pinned: the frame being pushed, max_out output frames, t, the scene result
    StreamMem sm;
    int64_t in_bytes, slot_bytes, out_bytes, ws_bytes;
    uint8_t* raw;
    uint8_t* slot[2];
    uint8_t* fwd_out;
    uint8_t* out_dev;
    float* t_dev;
    void* state_dev;
    void* ws;
    uint8_t* in_host;
    uint8_t* out_host;
    float* t_host;
    fldr_scene_result* scene_host;
    int64_t n;                         // frames pushed since create / reset
    int64_t j;                         // the next output frame
};

namespace {

void forget(fldr_scale* s) { s->n = 0; s->j = 0; }

fldr_video_frame slot_frame(const fldr_scale* s, uint8_t* base) { return padded(base, s->cfg.rate.format, s->fH, s->fW); }

fldr_video_frame out_frame(const fldr_scale* s, uint8_t* base) { return padded(base, s->cfg.rate.format, s->cfg.out_H, s->cfg.out_W); }

// Output k of a call, which lives at `src` at the size of the slots: scaled first under AFTER, then enqueued to pinned output frame k
int enqueue_output(fldr_scale* s, int k, uint8_t* src) {
    const uint8_t* from = src;
    if (!s->before) {
        uint8_t* dst = s->out_dev + k * s->out_bytes;
        CK(enqueue_scale(s->map, slot_frame(s, src), out_frame(s, dst), s->sm.stream));
        from = dst;
    }
    return (int)hipMemcpyAsync(s->out_host + k * s->out_bytes, from, (size_t)s->out_bytes, hipMemcpyDeviceToHost, s->sm.stream);
}

// the end of a call whose enqueues came to `rc`: the wait, and on success the first `count` pinned output frames go to host_outs
int finish(fldr_scale* s, int rc, const fldr_video_frame* host_outs, int count) {
    const hipError_t e = hipStreamSynchronize(s->sm.stream);
    if (!rc) rc = (int)e;
    if (rc) { (void)hipGetLastError(); forget(s); return rc; }
    const fldr_scale_config& c = s->cfg;
    for (int k = 0; k < count; ++k) copy_planes(host_outs[k], out_frame(s, s->out_host + k * s->out_bytes), c.rate.format, c.out_H, c.out_W);
    return 0;
}

}  // namespace

extern "C" FLDR_SCALE_API int fldr_scale_create(const fldr_model* m, fldr_scale_config* cfg, fldr_scale** out) {
    if (!cfg || !out) return FLDR_RATE_E_ARG;
    *out = nullptr;
    const fldr_rate_config& r = cfg->rate;
    CK(check_rate_config(r));
    RatePlan plan;
    CK(reduce_rate(r.in_num, r.in_den, r.out_num, r.out_den, plan));
    CK(check_scale_words(r.H, r.W, cfg->out_H, cfg->out_W, cfg->filter, cfg->where, cfg->reserved, 4, true));
    const bool forwards = plan.B != 1;
    if (forwards && !m) return FLDR_RATE_E_ARG;
    const int where = resolve_where(cfg->where, r.H, r.W, cfg->out_H, cfg->out_W);
    const bool before = where == FLDR_SCALE_BEFORE;
    const int fH = before ? cfg->out_H : r.H, fW = before ? cfg->out_W : r.W;
    const int64_t wsb = forwards ? fldr_rate_workspace_bytes(m, fH, fW, plan.max_out) : 0;
    if (wsb < 0) return (int)wsb;
    if (!device_exists(r.device)) return FLDR_RATE_E_DEVICE;
    fldr_scale* s = new (std::nothrow) fldr_scale();
    if (!s) return FLDR_RATE_E_DEVICE;
    fldr_scale_map_config mc;
    memset(&mc, 0, sizeof(mc));
    mc.in_H = r.H; mc.in_W = r.W; mc.out_H = cfg->out_H; mc.out_W = cfg->out_W;
    mc.format = r.format; mc.filter = cfg->filter; mc.device = r.device; mc.where = where;
    const int rc = fldr_scale_map_create(&mc, &s->map);
    if (rc) { delete s; return rc; }
    s->model = m;
    s->cfg = *cfg;
    s->cfg.where = where;
    s->plan = plan;
    s->before = before; s->forwards = forwards;
    s->fH = fH; s->fW = fW;
    const int max_out = plan.max_out;
    s->in_bytes = align_up(padded_bytes(r.format, r.H, r.W));
    s->slot_bytes = align_up(padded_bytes(r.format, fH, fW));
    s->out_bytes = align_up(padded_bytes(r.format, cfg->out_H, cfg->out_W));
    s->ws_bytes = wsb;
    const int64_t t_bytes = align_up(4ll * max_out);
    const int64_t raw_bytes = before ? s->in_bytes : 0, fwd_bytes = forwards ? max_out * s->slot_bytes : 0;
    const int64_t scaled_bytes = before ? 0 : max_out * s->out_bytes;
    const int64_t dev_total = raw_bytes + 2 * s->slot_bytes + fwd_bytes + scaled_bytes + t_bytes + FLDR_SCENE_STATE_BYTES + wsb;
    const int64_t host_total = s->in_bytes + max_out * s->out_bytes + t_bytes + ALIGN;
    if (!open_stream_mem(s->sm, r.device, dev_total, host_total)) {
        fldr_scale_map_destroy(&s->map);
        delete s;
        return FLDR_RATE_E_DEVICE;
    }
    s->raw = s->sm.dev;
    s->slot[0] = s->raw + raw_bytes;
    s->slot[1] = s->slot[0] + s->slot_bytes;
    s->fwd_out = s->slot[1] + s->slot_bytes;
    s->out_dev = s->fwd_out + fwd_bytes;
    s->t_dev = (float*)(s->out_dev + scaled_bytes);
    s->state_dev = (uint8_t*)s->t_dev + t_bytes;
    s->ws = forwards ? (uint8_t*)s->state_dev + FLDR_SCENE_STATE_BYTES : nullptr;
    s->in_host = s->sm.pinned;
    s->out_host = s->in_host + s->in_bytes;
    s->t_host = (float*)(s->out_host + max_out * s->out_bytes);
    s->scene_host = (fldr_scene_result*)((uint8_t*)s->t_host + t_bytes);
    forget(s);
    cfg->where = where;
    *out = s;
    return 0;
}

extern "C" FLDR_SCALE_API int fldr_scale_max_out(const fldr_scale* s) { return s ? s->plan.max_out : FLDR_RATE_E_ARG; }

extern "C" FLDR_SCALE_API int fldr_scale_push(fldr_scale* s, const fldr_video_frame* frame, const fldr_video_frame* host_outs, int* n_out,
                                              fldr_scene_result* scene) {
    if (!s || !frame || !n_out) return FLDR_RATE_E_ARG;
    *n_out = 0;
    if (scene) memset(scene, 0, sizeof(*scene));
    const fldr_scale_config& c = s->cfg;
    const fldr_rate_config& r = c.rate;
    const fldr_video_format& fmt = r.format;
    CK(check_frame(*frame, fmt, r.W));
    const bool pair = s->n >= 1;
    int n_t = 0;
    int64_t r_of[FLDR_RATE_MAX_OUT];
    const int count = pair ? pair_outputs(s->plan, s->n, s->j, r_of, n_t) : 0;
    if (count) {
        if (!host_outs) return FLDR_RATE_E_ARG;
        for (int k = 0; k < count; ++k) CK(check_frame(host_outs[k], fmt, c.out_W));
    }
    DeviceGuard g(s->sm.device);
    if (!g.ok) return FLDR_RATE_E_DEVICE;
    const hipStream_t stream = s->sm.stream;
    uint8_t* cur = s->slot[s->n & 1];
    uint8_t* prev = s->slot[(s->n - 1) & 1];
    // the frame is uploaded once; under BEFORE it is scaled once, here, into its slot
    copy_planes(padded(s->in_host, fmt, r.H, r.W), *frame, fmt, r.H, r.W);
    int rc = (int)hipMemcpyAsync(s->before ? s->raw : cur, s->in_host, (size_t)s->in_bytes, hipMemcpyHostToDevice, stream);
    if (!rc && s->before) rc = enqueue_scale(s->map, padded(s->raw, fmt, r.H, r.W), slot_frame(s, cur), stream);
    const bool measure = pair && r.scene == 1;
    if (!rc && (n_t || measure)) {
        fldr_video_io io;
        memset(&io, 0, sizeof(io));
        io.H = s->fH; io.W = s->fW;
        io.in_format = io.out_format = fmt;
        io.in[0] = slot_frame(s, prev); io.in[1] = slot_frame(s, cur);
        void* state = s->state_dev;
        if (n_t) {
            fill_times(r_of, count, s->plan.B, s->t_host);
            rc = (int)hipMemcpyAsync(s->t_dev, s->t_host, 4ull * n_t, hipMemcpyHostToDevice, stream);
            fldr_video_frame outs[FLDR_RATE_MAX_OUT];
            for (int q = 0; q < n_t; ++q) outs[q] = slot_frame(s, s->fwd_out + q * s->slot_bytes);
            io.n_t = n_t; io.t = s->t_dev; io.out = outs;
            if (!rc && measure) {
                // the forward always runs; on a cut the select of fldr_rate_forward overwrites its outputs on the device
                const int64_t need = fldr_rate_workspace_bytes(s->model, s->fH, s->fW, n_t);
                rc = need < 0 ? (int)need : fldr_rate_forward(s->model, &io, &r.scene_params, s->ws, s->ws_bytes, stream);
                state = (uint8_t*)s->ws + need - FLDR_SCENE_STATE_BYTES;
            } else if (!rc) {
                rc = fldr_video_forward(s->model, &io, s->ws, s->ws_bytes, stream);
            }
        } else {
            rc = fldr_scene_measure(s->fH, s->fW, &fmt, io.in, &r.scene_params, state, stream);      // a pair without an interpolated output
        }
        if (!rc && measure) rc = (int)hipMemcpyAsync(s->scene_host, state, sizeof(fldr_scene_result), hipMemcpyDeviceToHost, stream);
    }
    for (int k = 0, q = 0; k < count && !rc; ++k) rc = enqueue_output(s, k, r_of[k] ? s->fwd_out + (q++) * s->slot_bytes : prev);
    rc = finish(s, rc, host_outs, count);
    if (rc) return rc;
    if (measure && scene) *scene = *s->scene_host;
    *n_out = count;
    s->j += count;
    s->n += 1;
    return 0;
}

extern "C" FLDR_SCALE_API int fldr_scale_flush(fldr_scale* s, const fldr_video_frame* host_outs, int* n_out) {
    if (!s || !n_out) return FLDR_RATE_E_ARG;
    *n_out = 0;
    if (!s->n || !flush_due(s->plan, s->n, s->j)) return 0;
    if (!host_outs) return FLDR_RATE_E_ARG;
    CK(check_frame(host_outs[0], s->cfg.rate.format, s->cfg.out_W));
    DeviceGuard g(s->sm.device);
    if (!g.ok) return FLDR_RATE_E_DEVICE;
    int rc = enqueue_output(s, 0, s->slot[(s->n - 1) & 1]);
    rc = finish(s, rc, host_outs, 1);
    if (rc) return rc;
    s->j += 1;
    *n_out = 1;
    return 0;
}

extern "C" FLDR_SCALE_API int fldr_scale_reset(fldr_scale* s) {
    if (!s) return FLDR_RATE_E_ARG;
    forget(s);
    return 0;
}

extern "C" FLDR_SCALE_API void fldr_scale_destroy(fldr_scale* s) {
    if (!s) return;
    close_stream_mem(s->sm);
    fldr_scale_map_destroy(&s->map);
    delete s;
}
