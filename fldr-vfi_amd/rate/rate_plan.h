// The host text the rate family shares: what a valid fldr_rate_config is, the reduced ratio of its rates, which outputs a frame pair
// has, and the device work of a pair.  Included by rate_host.hip, ../pipe/pipe_host.hip and ../cadence/cadence_host.hip: the pipe is
// the converter with frames in flight and the cadence stream refuses exactly what fldr_rate_create refuses because all three compile
// this text.  Everything is in the unnamed namespace, as in ../video/frame_host.h: nothing here becomes a symbol of a library.
#pragma once
#include "../video/frame_host.h"
#include "fldr_rate.h"

namespace {

// the one statement of the thresholds' rule: FLDR_RATE_E_ARG outside 0 .. 1000 or with a reserved word set
int check_scene_params(const fldr_scene_params& p) {
    if (p.sad_permille < 0 || p.sad_permille > 1000 || p.hist_permille < 0 || p.hist_permille > 1000) return FLDR_RATE_E_ARG;
    if (p.reserved[0] || p.reserved[1]) return FLDR_RATE_E_ARG;
    return 0;
}

// fldr_rate_create's checks of a configuration, in its order and with its codes, up to the rate terms being positive
int check_rate_config(const fldr_rate_config& c) {
    if (c.H < 2 || c.W < 2 || c.device < 0 || (unsigned)c.scene > 1u) return FLDR_RATE_E_ARG;
    for (int i = 0; i < 4; ++i) if (c.reserved[i]) return FLDR_RATE_E_ARG;
    CK(check_scene_params(c.scene_params));
    CK(check_format(c.format));
    if (c.in_num <= 0 || c.in_den <= 0 || c.out_num <= 0 || c.out_den <= 0) return FLDR_RATE_E_RATIO;
    return 0;
}

int64_t gcd64(int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; }

void reduce_terms(int64_t& n, int64_t& d) { const int64_t g = gcd64(n, d); n /= g; d /= g; }

struct RatePlan {
    int64_t A, B;                      // output j at input position j A / B
    int max_out;                       // ceil(B / A): the most outputs one pair has
};

// positive A / B, input frames per output -> the plan; FLDR_RATE_E_RATIO for a ratio outside what the converter takes
int plan_of_ratio(int64_t A, int64_t B, RatePlan& p) {
    reduce_terms(A, B);
    // t = (float)r / (float)B is then exact in its operands, and t < 0.5f exactly where r * 2 < B
    if (A > (1ll << 24) || B > (1ll << 24) || (B + A - 1) / A > FLDR_RATE_MAX_OUT) return FLDR_RATE_E_RATIO;
    p.A = A; p.B = B; p.max_out = (int)((B + A - 1) / A);
    return 0;
}

// positive rate terms -> the plan
int reduce_rate(int32_t in_num, int32_t in_den, int32_t out_num, int32_t out_den, RatePlan& p) {
    return plan_of_ratio((int64_t)in_num * out_den, (int64_t)in_den * out_num, p);
}

// The outputs of the pair (n - 1, n), by fldr_rate.h's rule: every j from the next output on with (n - 1) B <= j A < n B;
// r_of[k] = j A - (n - 1) B, 0 where the output is frame n - 1 itself.  -> their number; n_t: those with r != 0, the interpolated ones
int pair_outputs(const RatePlan& p, int64_t n, int64_t j, int64_t r_of[FLDR_RATE_MAX_OUT], int& n_t) {
    int count = n_t = 0;
    for (; j * p.A < n * p.B && count < FLDR_RATE_MAX_OUT; ++j) {
        r_of[count] = j * p.A - (n - 1) * p.B;
        if (r_of[count]) ++n_t;
        ++count;
    }
    return count;
}

// at the end of a stream of n frames: the next output lands exactly on the last frame
bool flush_due(const RatePlan& p, int64_t n, int64_t j) { return j * p.A == (n - 1) * p.B; }

// t of the interpolated outputs, in order
void fill_times(const int64_t* r_of, int count, int64_t B, float* t_host) {
    for (int k = 0, q = 0; k < count; ++k) if (r_of[k]) t_host[q++] = (float)r_of[k] / (float)B;
}

// The device work of a pair with n_t interpolated outputs or a measure (c.scene), enqueued on `stream`: the packed device frames in0, in1
// -> n_t packed frames from out_base on, at the times t_dev, and the fldr_scene_result -> scene_dst (pinned).  state_dev serves a pair
// without an interpolated output; otherwise the scene state is the one inside the workspace.
int enqueue_pair(const fldr_model* m, const fldr_rate_config& c, int n_t, uint8_t* in0, uint8_t* in1, uint8_t* out_base, int64_t frame_bytes,
                 const float* t_dev, void* ws, int64_t ws_bytes, void* state_dev, void* scene_dst, hipStream_t stream) {
    const int H = c.H, W = c.W;
    const fldr_video_format& fmt = c.format;
    const bool measure = c.scene == 1;
    const fldr_video_frame in[2] = { packed(in0, fmt, H, W), packed(in1, fmt, H, W) };
    void* state = state_dev;
    if (n_t) {
        fldr_video_frame outs[FLDR_RATE_MAX_OUT];
        for (int k = 0; k < n_t; ++k) outs[k] = packed(out_base + k * frame_bytes, fmt, H, W);
        fldr_video_io io;
        memset(&io, 0, sizeof(io));
        io.H = H; io.W = W;
        io.in_format = io.out_format = fmt;
        io.in[0] = in[0]; io.in[1] = in[1];
        io.n_t = n_t; io.t = t_dev; io.out = outs;
        if (measure) {
            // the forward always runs; on a cut the select of fldr_rate_forward overwrites its outputs on the device
            const int64_t need = fldr_rate_workspace_bytes(m, H, W, n_t);
            if (need < 0) return (int)need;
            CK(fldr_rate_forward(m, &io, &c.scene_params, ws, ws_bytes, stream));
            state = (char*)ws + need - FLDR_SCENE_STATE_BYTES;
        } else {
            CK(fldr_video_forward(m, &io, ws, ws_bytes, stream));
        }
    } else {
        CK(fldr_scene_measure(H, W, &fmt, in, &c.scene_params, state, stream));            // a pair without an interpolated output
    }
    return measure ? (int)hipMemcpyAsync(scene_dst, state, sizeof(fldr_scene_result), hipMemcpyDeviceToHost, stream) : 0;
}

}  // namespace
