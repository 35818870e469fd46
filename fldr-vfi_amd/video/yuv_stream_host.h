// A frame library on the model library, host side, written once: the checks of a forward's arguments, the workspace layout, the forward
// (input conversion -> one fldr_model_forward -> n_t output conversions -> the library's pass over the outputs, if it has one), the
// session for streams of host frames, and what the exported functions of every such library share: the two converters alone, the
// struct sizes and the tail of the error strings.  Included first by video_host.hip (4:2:0), ../chroma/chroma_host.hip (4:2:2, 4:4:4),
// ../pack10/pack10_host.hip (v210, Y210, Y410) and ../rgb/rgb_host.hip (RGB with alpha); each states the FrameRules of its format
// (frame_host.h) and instantiates this text with a traits struct L : LibDefaults that names
//   Format, Frame, Io, Config                       the library's C structs (Io and Config laid out as fldr_video_io / _session_config)
//   E_ARG, E_FORMAT, E_WORKSPACE, E_DEVICE          its error codes (E_PLANE and E_PITCH are in its FrameRules)
//   check_format(fmt)                               what a valid format is
//   to_planar(in, n, fmt, planar, H, W, stream)     n (1 .. MAX_FRAMES) frames -> planar BGR [n,3,H,W]
//   from_planar(planar, out, fmt, H, W, stream)     one planar BGR frame -> one frame
// and, where it has them (LibDefaults has the no-op forms),
//   check_pair(in_format, out_format)               which valid formats may meet in one forward
//   after_outputs(io, stream)                       a pass after the n_t output conversions of a forward
// and, where it exports the converters (libfldr_video.so does not),
//   MAX_FRAMES                                      frames one input launch converts
// and derives its opaque session struct from Session<L>.  Everything is in the unnamed namespace, like frame_host.h: nothing here
// becomes a symbol of any library.  The only fldr_* functions called are those of fldr_model.h.
#pragma once
#include <new>
#include <vector>

#include "fldr_model.h"
#include "frame_host.h"

namespace {

// what a traits struct may leave out
struct LibDefaults {
    template <class Format> static int check_pair(const Format&, const Format&) { return 0; }
    template <class Io> static int after_outputs(const Io&, hipStream_t) { return 0; }
};

// host-only checks of a forward's arguments (no model, no device)
template <class L> int validate_io(const typename L::Io* io) {
    if (!io) return L::E_ARG;
    if (io->H < 2 || io->W < 2 || io->n_t < 1 || !io->t || !io->out) return L::E_ARG;
    int rc = L::check_format(io->in_format);
    if (!rc) rc = L::check_format(io->out_format);
    for (int f = 0; f < 2 && !rc; ++f) rc = check_frame(io->in[f], io->in_format, io->W);
    for (int k = 0; k < io->n_t && !rc; ++k) rc = check_frame(io->out[k], io->out_format, io->W);
    return rc;
}

struct WsLayout { int64_t model, pair, out, out_stride, total; };

// in_bytes / out_bytes: bytes per sample of the planar pair / outputs of THIS forward (the offsets); the total is always that of the
// 16-bit regions, so one size serves every format (the *_workspace_bytes functions have no format argument)
template <class L> int64_t plan(const fldr_model* m, int H, int W, int n_t, int in_bytes, int out_bytes, WsLayout& ws) {
    if (!m || H < 2 || W < 2 || n_t < 1) return L::E_ARG;
    const int64_t mb = fldr_model_workspace_bytes(m, H, W, n_t);
    if (mb < 0) return mb;
    ws.model = 0;
    ws.pair = align_up(mb);
    ws.out = ws.pair + align_up(6ll * H * W * in_bytes);
    ws.out_stride = align_up(3ll * H * W * out_bytes);
    ws.total = ws.pair + align_up(12ll * H * W) + (int64_t)n_t * align_up(6ll * H * W);
    return ws.total;
}

template <class L> int64_t workspace_bytes(const fldr_model* m, int H, int W, int n_t) {
    WsLayout ws;
    return plan<L>(m, H, W, n_t, 2, 2, ws);
}

template <class L> int forward(const fldr_model* m, const typename L::Io* io, void* ws, int64_t ws_bytes, void* stream) {
    CK(validate_io<L>(io));
    CK(L::check_pair(io->in_format, io->out_format));
    WsLayout lay;
    const bool in10 = deep(io->in_format), out10 = deep(io->out_format);
    const int64_t total = plan<L>(m, io->H, io->W, io->n_t, in10 ? 2 : 1, out10 ? 2 : 1, lay);
    if (total < 0) return (int)total;
    if (!ws || ((uintptr_t)ws & (ALIGN - 1)) || ws_bytes < total) return L::E_WORKSPACE;
    const int H = io->H, W = io->W;
    char* w = (char*)ws;
    void* pair = w + lay.pair;
    const hipStream_t s = (hipStream_t)stream;
    std::vector<void*> planar((size_t)io->n_t);
    for (int k = 0; k < io->n_t; ++k) planar[k] = w + lay.out + (int64_t)k * lay.out_stride;
    // the conversion writes the workspace only: if the model then refuses (a fault flag of an earlier call), no output is touched
    CK(L::to_planar(io->in, 2, io->in_format, pair, H, W, s));
    fldr_model_io mio;
    memset(&mio, 0, sizeof(mio));
    mio.batch = 1; mio.H = H; mio.W = W; mio.input = in10 ? FLDR_MODEL_IN_U10_PLANAR : FLDR_MODEL_IN_U8_PLANAR; mio.frames_u8 = (const uint8_t*)pair;
    mio.n_t = io->n_t; mio.t = io->t; mio.output = out10 ? FLDR_MODEL_OUT_U10_PLANAR : FLDR_MODEL_OUT_U8_PLANAR; mio.out = planar.data();
    CK(fldr_model_forward(m, &mio, w + lay.model, lay.pair, stream));
    for (int k = 0; k < io->n_t; ++k) CK(L::from_planar(planar[k], io->out[k], io->out_format, H, W, s));
    return L::after_outputs(*io, s);
}

// ---- sessions -----------------------------------------------------------------------------------------------------------------
template <class L> struct Session {
    const fldr_model* model;
    typename L::Config cfg;
    StreamMem sm;                      // device: slot 0, slot 1, n_t outputs, t, workspace; pinned: one input frame, n_t output frames (packed)
    int64_t in_bytes, out_bytes, ws_bytes;
    uint8_t* slot[2];
    uint8_t* out_dev;
    float* t_dev;
    void* ws;
    int prev;                          // slot holding the previous frame, -1 when none
};

template <class S> void session_destroy(S* s) {
    if (s) { close_stream_mem(s->sm); delete s; }
}

// S: the library's session struct, a Session<L>
template <class L, class S> int session_create(const fldr_model* m, const typename L::Config* cfg, S** out) {
    if (!cfg || !out) return L::E_ARG;
    *out = nullptr;
    if (cfg->H < 2 || cfg->W < 2 || cfg->n_t < 1 || cfg->device < 0) return L::E_ARG;
    CK(L::check_format(cfg->in_format));
    CK(L::check_format(cfg->out_format));
    CK(L::check_pair(cfg->in_format, cfg->out_format));
    for (int i = 0; i < 4; ++i) if (cfg->reserved[i]) return L::E_FORMAT;
    if (!m) return L::E_ARG;
    const int H = cfg->H, W = cfg->W, n_t = cfg->n_t;
    const int64_t wsb = workspace_bytes<L>(m, H, W, n_t);
    if (wsb < 0) return (int)wsb;
    if (!device_exists(cfg->device)) return L::E_DEVICE;
    S* s = new (std::nothrow) S();
    if (!s) return L::E_DEVICE;
    s->model = m;
    s->cfg = *cfg;
    s->cfg.t = nullptr;
    s->prev = -1;
    s->in_bytes = align_up(packed_bytes(cfg->in_format, H, W));
    s->out_bytes = align_up(packed_bytes(cfg->out_format, H, W));
    s->ws_bytes = wsb;
    DeviceGuard g(cfg->device);
    const int64_t dev_total = 2 * s->in_bytes + n_t * s->out_bytes + align_up(4ll * n_t) + wsb;
    const int64_t host_total = s->in_bytes + n_t * s->out_bytes;
    if (!g.ok || !open_stream_mem(s->sm, cfg->device, dev_total, host_total)) { delete s; return L::E_DEVICE; }
    s->slot[0] = s->sm.dev;
    s->slot[1] = s->slot[0] + s->in_bytes;
    s->out_dev = s->slot[1] + s->in_bytes;
    s->t_dev = (float*)(s->out_dev + n_t * s->out_bytes);
    s->ws = (char*)s->t_dev + align_up(4ll * n_t);
    std::vector<float> t((size_t)n_t);
    for (int k = 0; k < n_t; ++k) t[k] = cfg->t ? cfg->t[k] : (float)(k + 1) / (float)(n_t + 1);
    hipError_t e = hipMemcpyAsync(s->t_dev, t.data(), 4ull * n_t, hipMemcpyHostToDevice, s->sm.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->sm.stream);
    if (e != hipSuccess) { session_destroy(s); return (int)e; }
    *out = s;
    return 0;
}

template <class L> int session_push(Session<L>* s, const typename L::Frame* frame, const typename L::Frame* host_outs, int* n_out) {
    if (!s || !frame || !n_out) return L::E_ARG;
    *n_out = 0;
    const typename L::Config& c = s->cfg;
    const int H = c.H, W = c.W, n_t = c.n_t;
    CK(check_frame(*frame, c.in_format, W));
    if (s->prev >= 0) {
        if (!host_outs) return L::E_ARG;
        for (int k = 0; k < n_t; ++k) CK(check_frame(host_outs[k], c.out_format, W));
    }
    DeviceGuard g(s->sm.device);
    if (!g.ok) return L::E_DEVICE;
    const hipStream_t stream = s->sm.stream;
    const int cur = s->prev == 0 ? 1 : 0;                          // the slot not holding the previous frame
    hipError_t e = upload_frame(s->sm, s->slot[cur], s->sm.pinned, s->in_bytes, *frame, c.in_format, H, W);
    int rc = e == hipSuccess ? 0 : (int)e;
    const bool interp = s->prev >= 0;
    uint8_t* out_host = s->sm.pinned + s->in_bytes;
    if (!rc && interp) {
        std::vector<typename L::Frame> outs((size_t)n_t);
        for (int k = 0; k < n_t; ++k) outs[k] = packed(s->out_dev + k * s->out_bytes, c.out_format, H, W);
        typename L::Io io;
        memset(&io, 0, sizeof(io));
        io.H = H; io.W = W;
        io.in_format = c.in_format;
        io.in[0] = packed(s->slot[s->prev], c.in_format, H, W);
        io.in[1] = packed(s->slot[cur], c.in_format, H, W);
        io.out_format = c.out_format;
        io.n_t = n_t; io.t = s->t_dev; io.out = outs.data();
        rc = forward<L>(s->model, &io, s->ws, s->ws_bytes, stream);
        if (!rc) {
            e = hipMemcpyAsync(out_host, s->out_dev, (size_t)(n_t * s->out_bytes), hipMemcpyDeviceToHost, stream);
            if (e != hipSuccess) rc = (int)e;
        }
    }
    e = hipStreamSynchronize(stream);
    if (!rc && e != hipSuccess) rc = (int)e;
    if (rc) { s->prev = -1; return rc; }                           // the held frame is not to be trusted
    if (interp) {
        for (int k = 0; k < n_t; ++k) unpack_frame(host_outs[k], out_host + k * s->out_bytes, c.out_format, H, W);
        *n_out = n_t;
    }
    s->prev = cur;
    return 0;
}

template <class L> int session_reset(Session<L>* s) {
    if (!s) return L::E_ARG;
    s->prev = -1;
    return 0;
}

// ---- what the exported functions share ----------------------------------------------------------------------------------------------
// The converters alone, as a library exports them (any size from 1 x 1, any number of frames; planar BGR of 16-bit samples at an even
// address): the checks, then one launch per MAX_FRAMES frames.
template <class L>
int to_planar_entry(const typename L::Frame* frames, int n_frames, const typename L::Format* format, void* planar, int H, int W, void* stream) {
    if (!frames || !format || !planar || n_frames < 1 || H < 1 || W < 1) return L::E_ARG;
    CK(L::check_format(*format));
    if (deep(*format) && ((uintptr_t)planar & 1)) return L::E_ARG;
    for (int f = 0; f < n_frames; ++f) CK(check_frame(frames[f], *format, W));
    const int64_t frame_bytes = 3ll * H * W * (deep(*format) ? 2 : 1);
    for (int f = 0; f < n_frames; f += L::MAX_FRAMES) {
        const int n = n_frames - f < L::MAX_FRAMES ? n_frames - f : L::MAX_FRAMES;
        CK(L::to_planar(frames + f, n, *format, (uint8_t*)planar + f * frame_bytes, H, W, (hipStream_t)stream));
    }
    return 0;
}

template <class L>
int from_planar_entry(const void* planar, const typename L::Format* format, const typename L::Frame* out_frame, int H, int W, void* stream) {
    if (!planar || !format || !out_frame || H < 1 || W < 1) return L::E_ARG;
    CK(L::check_format(*format));
    if (deep(*format) && ((uintptr_t)planar & 1)) return L::E_ARG;
    CK(check_frame(*out_frame, *format, W));
    return L::from_planar(planar, *out_frame, *format, H, W, (hipStream_t)stream);
}

// fldr_*_sizeof: the sizes of the four structs, for a binding to check itself against
template <class L> int struct_sizeof(int which) {
    switch (which) {
    case 0: return (int)sizeof(typename L::Format);
    case 1: return (int)sizeof(typename L::Frame);
    case 2: return (int)sizeof(typename L::Io);
    case 3: return (int)sizeof(typename L::Config);
    default: return L::E_ARG;
    }
}

// fldr_*_error_string for a code that is not the library's own: the model's, the HIP runtime's, or `unknown`
const char* passed_error_string(int code, const char* unknown) {
    return code > -100 && code < 0 ? fldr_model_error_string(code) : code > 0 ? hipGetErrorString((hipError_t)code) : unknown;
}

}  // namespace
