// libfldr_pipe.so: the rate converter with frames in flight (include/fldr_pipe.h).  Host code only — there is no kernel here: a job's
// device work is fldr_rate_forward / fldr_video_forward / fldr_scene_measure, as fldr_rate_push enqueues it, between an upload on one
// stream and a download on another.  The converter's configuration rules, its schedule and that device work are the text of
// ../rate/rate_plan.h, compiled here as in the rate library; the video API's rules for formats and frames come with it from
// ../video/frame_host.h.  The only fldr_* functions called are those of fldr_rate.h, fldr_video.h and fldr_model.h.
#include <hip/hip_runtime.h>

#include <cstring>
#include <initializer_list>
#include <new>

#include "../rate/rate_plan.h"
#include "fldr_pipe.h"

namespace {

constexpr int64_t T_BYTES = 256;                       // FLDR_RATE_MAX_OUT floats
constexpr int64_t SCENE_BYTES = 256;                   // a fldr_scene_result, on a line of its own
static_assert(T_BYTES == 4 * FLDR_RATE_MAX_OUT && sizeof(fldr_scene_result) <= SCENE_BYTES, "per-job slots");

struct Job {
    int count;                         // outputs
    int n_t;                           // of them interpolated: frames in the job's output set, in order
    bool waits;                        // an event to wait for (every submit; a flush enqueues nothing)
    bool scene;                        // the pair was measured: the job's pinned scene slot holds the result
    int in_slot;                       // pinned input slot of frame n - 1: the bytes of the r == 0 outputs
    int out_set;                       // pinned output set
    uint64_t direct;                   // bit k: output k is frame n - 1 itself (r == 0)
};

}  // namespace

struct fldr_pipe {
    const fldr_model* model;
    fldr_rate_config cfg;
    int depth;
    RatePlan plan;
    int device;
    hipStream_t up, comp, down;
    hipEvent_t ev_up[FLDR_PIPE_MAX_DEPTH], ev_comp[FLDR_PIPE_MAX_DEPTH], ev_down[FLDR_PIPE_MAX_DEPTH];   // by job number mod depth
    uint8_t* dev;
    uint8_t* pinned;
    int64_t frame_bytes, ws_bytes;
    int n_in_dev, n_in_host, n_out_host;                       // ring lengths: depth + 1, depth + 3, depth + 1
    uint8_t *in_dev, *out_dev, *t_dev, *state_dev, *ws;        // device block
    uint8_t *in_host, *out_host, *t_host, *scene_host;         // pinned block
    Job jobs[FLDR_PIPE_MAX_DEPTH];
    int64_t job_seq;                   // jobs created since create: job k lives in jobs[k % depth]
    int pending;                       // the oldest outstanding job is job_seq - pending
    int64_t in_seq;                    // frames submitted since create: the ring position of the next frame
    int prev_dev, prev_host;           // device / pinned slot of frame n - 1, -1 when none
    int64_t n, j;                      // frames submitted since create / reset, the next output frame
};

namespace {

void fresh_stream(fldr_pipe* p) { p->pending = 0; p->prev_dev = p->prev_host = -1; p->n = 0; p->j = 0; }

// wait for everything enqueued and forget it; -> the first error of the three waits
int drain(fldr_pipe* p) {
    int rc = 0;
    for (hipStream_t s : { p->up, p->comp, p->down }) {
        const hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess && !rc) rc = (int)e;
    }
    if (rc) (void)hipGetLastError();
    fresh_stream(p);
    return rc;
}

void close_pipe(fldr_pipe* p) {
    DeviceGuard g(p->device);
    for (hipStream_t s : { p->up, p->comp, p->down }) if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
    for (int k = 0; k < FLDR_PIPE_MAX_DEPTH; ++k)
        for (hipEvent_t e : { p->ev_up[k], p->ev_comp[k], p->ev_down[k] }) if (e) (void)hipEventDestroy(e);
    if (p->dev) (void)hipFree(p->dev);
    if (p->pinned) (void)hipHostFree(p->pinned);
    (void)hipGetLastError();
    delete p;
}

#define HIPRC(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

// everything a submit enqueues; the job record is complete when it is called
int enqueue_push(fldr_pipe* p, const Job& job, int slot, int cur_dev, int cur_host, const int64_t* r_of) {
    float* t_host = (float*)(p->t_host + slot * T_BYTES);
    float* t_dev = (float*)(p->t_dev + slot * T_BYTES);
    if (job.n_t) {
        fill_times(r_of, job.count, p->plan.B, t_host);
        HIPRC(hipMemcpyAsync(t_dev, t_host, 4ull * job.n_t, hipMemcpyHostToDevice, p->up));
    }
    HIPRC(hipMemcpyAsync(p->in_dev + cur_dev * p->frame_bytes, p->in_host + cur_host * p->frame_bytes, (size_t)p->frame_bytes,
                         hipMemcpyHostToDevice, p->up));
    HIPRC(hipEventRecord(p->ev_up[slot], p->up));
    HIPRC(hipStreamWaitEvent(p->comp, p->ev_up[slot], 0));
    if (p->prev_dev >= 0 && (job.n_t || job.scene))
        CK(enqueue_pair(p->model, p->cfg, job.n_t, p->in_dev + p->prev_dev * p->frame_bytes, p->in_dev + cur_dev * p->frame_bytes,
                        p->out_dev + (int64_t)slot * p->plan.max_out * p->frame_bytes, p->frame_bytes, t_dev, p->ws, p->ws_bytes, p->state_dev,
                        p->scene_host + slot * SCENE_BYTES, p->comp));
    HIPRC(hipEventRecord(p->ev_comp[slot], p->comp));
    HIPRC(hipStreamWaitEvent(p->down, p->ev_comp[slot], 0));
    if (job.n_t)
        HIPRC(hipMemcpyAsync(p->out_host + (int64_t)job.out_set * p->plan.max_out * p->frame_bytes,
                             p->out_dev + (int64_t)slot * p->plan.max_out * p->frame_bytes, (size_t)(job.n_t * p->frame_bytes),
                             hipMemcpyDeviceToHost, p->down));
    HIPRC(hipEventRecord(p->ev_down[slot], p->down));
    return 0;
}

// the oldest job, waited for: 0, FLDR_PIPE_E_EMPTY, or the wait's error after a drain
int wait_oldest(fldr_pipe* p, const Job*& job, int& slot) {
    if (!p->pending) return FLDR_PIPE_E_EMPTY;
    slot = (int)((p->job_seq - p->pending) % p->depth);
    job = &p->jobs[slot];
    if (job->waits) {
        const hipError_t e = hipEventSynchronize(p->ev_down[slot]);
        if (e != hipSuccess) { (void)hipGetLastError(); (void)drain(p); return (int)e; }
    }
    return 0;
}

// output k of a job, packed in pinned memory
uint8_t* output_of(const fldr_pipe* p, const Job& job, int k, int& q) {
    if (job.direct >> k & 1) return p->in_host + job.in_slot * p->frame_bytes;
    return p->out_host + ((int64_t)job.out_set * p->plan.max_out + q++) * p->frame_bytes;
}

void take_scene(const fldr_pipe* p, const Job& job, int slot, fldr_scene_result* scene) {
    if (!scene) return;
    if (job.scene) memcpy(scene, p->scene_host + slot * SCENE_BYTES, sizeof(*scene));
    else memset(scene, 0, sizeof(*scene));
}

}  // namespace

extern "C" FLDR_PIPE_API int fldr_pipe_version(void) { return FLDR_PIPE_VERSION; }

extern "C" FLDR_PIPE_API const char* fldr_pipe_error_string(int code) {
    switch (code) {
    case FLDR_PIPE_E_ARG: return "fldr_pipe: bad argument";
    case FLDR_PIPE_E_FULL: return "fldr_pipe: depth jobs are outstanding";
    case FLDR_PIPE_E_EMPTY: return "fldr_pipe: no job is outstanding";
    case FLDR_PIPE_E_DEVICE: return "fldr_pipe: no such device or out of memory";
    default: return code > -300 ? fldr_rate_error_string(code) : "fldr_pipe: unknown error";
    }
}

extern "C" FLDR_PIPE_API int fldr_pipe_sizeof(int which) {
    switch (which) {
    case 0: return (int)sizeof(fldr_pipe_config);
    default: return FLDR_PIPE_E_ARG;
    }
}

extern "C" FLDR_PIPE_API int fldr_pipe_create(const fldr_model* m, const fldr_pipe_config* pcfg, fldr_pipe** out) {
    if (!pcfg || !out) return FLDR_PIPE_E_ARG;
    *out = nullptr;
    // fldr_rate_create's checks, in its order and with its codes: ../rate/rate_plan.h
    const fldr_rate_config* cfg = &pcfg->rate;
    CK(check_rate_config(*cfg));
    RatePlan plan;
    CK(reduce_rate(cfg->in_num, cfg->in_den, cfg->out_num, cfg->out_den, plan));
    const int max_out = plan.max_out;
    // this library's
    if (pcfg->depth < 1 || pcfg->depth > FLDR_PIPE_MAX_DEPTH) return FLDR_PIPE_E_ARG;
    for (int i = 0; i < 3; ++i) if (pcfg->reserved[i]) return FLDR_PIPE_E_ARG;
    if (!m) return FLDR_PIPE_E_ARG;
    const int H = cfg->H, W = cfg->W, D = pcfg->depth;
    const int64_t wsb = fldr_rate_workspace_bytes(m, H, W, max_out);
    if (wsb < 0) return (int)wsb;
    if (!device_exists(cfg->device)) return FLDR_PIPE_E_DEVICE;
    fldr_pipe* p = new (std::nothrow) fldr_pipe();
    if (!p) return FLDR_PIPE_E_DEVICE;
    p->model = m;
    p->cfg = *cfg;
    p->depth = D;
    p->plan = plan;
    p->device = cfg->device;
    p->job_seq = 0; p->in_seq = 0;
    fresh_stream(p);
    const int64_t F = p->frame_bytes = align_up(packed_bytes(cfg->format, H, W));
    p->ws_bytes = wsb;
    p->n_in_dev = D + 1; p->n_in_host = D + 3; p->n_out_host = D + 1;
    const int64_t dev_total = (p->n_in_dev + (int64_t)D * max_out) * F + D * T_BYTES + FLDR_SCENE_STATE_BYTES + wsb;
    const int64_t host_total = (p->n_in_host + (int64_t)p->n_out_host * max_out) * F + D * T_BYTES + D * SCENE_BYTES;
    DeviceGuard guard(cfg->device);
    bool ok = guard.ok && hipMalloc((void**)&p->dev, (size_t)dev_total) == hipSuccess &&
              hipHostMalloc((void**)&p->pinned, (size_t)host_total, hipHostMallocDefault) == hipSuccess;
    for (hipStream_t* s : { &p->up, &p->comp, &p->down }) ok = ok && hipStreamCreateWithFlags(s, hipStreamNonBlocking) == hipSuccess;
    for (int k = 0; k < D; ++k)
        for (hipEvent_t* e : { &p->ev_up[k], &p->ev_comp[k], &p->ev_down[k] }) ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
    if (!ok) { close_pipe(p); return FLDR_PIPE_E_DEVICE; }
    p->in_dev = p->dev;
    p->out_dev = p->in_dev + p->n_in_dev * F;
    p->t_dev = p->out_dev + (int64_t)D * max_out * F;
    p->state_dev = p->t_dev + D * T_BYTES;
    p->ws = p->state_dev + FLDR_SCENE_STATE_BYTES;
    p->in_host = p->pinned;
    p->out_host = p->in_host + p->n_in_host * F;
    p->t_host = p->out_host + (int64_t)p->n_out_host * max_out * F;
    p->scene_host = p->t_host + D * T_BYTES;
    *out = p;
    return 0;
}

extern "C" FLDR_PIPE_API int fldr_pipe_max_out(const fldr_pipe* p) { return p ? p->plan.max_out : FLDR_PIPE_E_ARG; }

extern "C" FLDR_PIPE_API int fldr_pipe_pending(const fldr_pipe* p) { return p ? p->pending : FLDR_PIPE_E_ARG; }

extern "C" FLDR_PIPE_API int fldr_pipe_input(fldr_pipe* p, fldr_video_frame* frame) {
    if (!p || !frame) return FLDR_PIPE_E_ARG;
    *frame = packed(p->in_host + (p->in_seq % p->n_in_host) * p->frame_bytes, p->cfg.format, p->cfg.H, p->cfg.W);
    return 0;
}

extern "C" FLDR_PIPE_API int fldr_pipe_submit(fldr_pipe* p, const fldr_video_frame* host_frame) {
    if (!p) return FLDR_PIPE_E_ARG;
    const fldr_rate_config& c = p->cfg;
    if (host_frame) CK(check_frame(*host_frame, c.format, c.W));
    if (p->pending >= p->depth) return FLDR_PIPE_E_FULL;
    const bool pair = p->prev_dev >= 0;
    Job job;
    memset(&job, 0, sizeof(job));
    int64_t r_of[FLDR_RATE_MAX_OUT];
    if (pair) job.count = pair_outputs(p->plan, p->n, p->j, r_of, job.n_t);
    for (int k = 0; k < job.count; ++k) if (!r_of[k]) job.direct |= 1ull << k;
    const int slot = (int)(p->job_seq % p->depth);
    const int cur_dev = (int)(p->in_seq % p->n_in_dev), cur_host = (int)(p->in_seq % p->n_in_host);
    job.waits = true;
    job.scene = pair && c.scene == 1;
    job.in_slot = p->prev_host;
    job.out_set = (int)(p->job_seq % p->n_out_host);
    if (host_frame) copy_planes(packed(p->in_host + cur_host * p->frame_bytes, c.format, c.H, c.W), *host_frame, c.format, c.H, c.W);
    DeviceGuard g(p->device);
    if (!g.ok) return FLDR_PIPE_E_DEVICE;
    const int rc = enqueue_push(p, job, slot, cur_dev, cur_host, r_of);
    if (rc) { (void)hipGetLastError(); (void)drain(p); return rc; }      // what was enqueued is not to be trusted: as after a reset
    p->jobs[slot] = job;
    p->job_seq += 1; p->pending += 1; p->in_seq += 1;
    p->j += job.count; p->n += 1;
    p->prev_dev = cur_dev; p->prev_host = cur_host;
    return 0;
}

extern "C" FLDR_PIPE_API int fldr_pipe_flush(fldr_pipe* p) {
    if (!p) return FLDR_PIPE_E_ARG;
    if (p->pending >= p->depth) return FLDR_PIPE_E_FULL;
    Job job;
    memset(&job, 0, sizeof(job));
    if (p->prev_host >= 0 && flush_due(p->plan, p->n, p->j)) {          // the output that lands exactly on the last frame: its bytes
        job.count = 1;
        job.direct = 1;
        job.in_slot = p->prev_host;
        p->j += 1;
    }
    p->jobs[p->job_seq % p->depth] = job;
    p->job_seq += 1; p->pending += 1;
    return 0;
}

extern "C" FLDR_PIPE_API int fldr_pipe_receive(fldr_pipe* p, const fldr_video_frame* host_outs, int* n_out, fldr_scene_result* scene) {
    if (!p || !n_out) return FLDR_PIPE_E_ARG;
    *n_out = 0;
    if (scene) memset(scene, 0, sizeof(*scene));
    if (!p->pending) return FLDR_PIPE_E_EMPTY;
    const fldr_rate_config& c = p->cfg;
    const Job& peek = p->jobs[(p->job_seq - p->pending) % p->depth];
    if (peek.count) {
        if (!host_outs) return FLDR_PIPE_E_ARG;
        for (int k = 0; k < peek.count; ++k) CK(check_frame(host_outs[k], c.format, c.W));
    }
    DeviceGuard g(p->device);
    if (!g.ok) return FLDR_PIPE_E_DEVICE;
    const Job* job;
    int slot;
    CK(wait_oldest(p, job, slot));
    for (int k = 0, q = 0; k < job->count; ++k) unpack_frame(host_outs[k], output_of(p, *job, k, q), c.format, c.H, c.W);
    take_scene(p, *job, slot, scene);
    *n_out = job->count;
    p->pending -= 1;
    return 0;
}

extern "C" FLDR_PIPE_API int fldr_pipe_receive_view(fldr_pipe* p, fldr_video_frame* views, int* n_out, fldr_scene_result* scene) {
    if (!p || !views || !n_out) return FLDR_PIPE_E_ARG;
    *n_out = 0;
    if (scene) memset(scene, 0, sizeof(*scene));
    DeviceGuard g(p->device);
    if (!g.ok) return FLDR_PIPE_E_DEVICE;
    const Job* job;
    int slot;
    CK(wait_oldest(p, job, slot));
    const fldr_rate_config& c = p->cfg;
    for (int k = 0, q = 0; k < job->count; ++k) views[k] = packed(output_of(p, *job, k, q), c.format, c.H, c.W);
    take_scene(p, *job, slot, scene);
    *n_out = job->count;
    p->pending -= 1;
    return 0;
}

extern "C" FLDR_PIPE_API int fldr_pipe_reset(fldr_pipe* p) {
    if (!p) return FLDR_PIPE_E_ARG;
    DeviceGuard g(p->device);
    if (!g.ok) return FLDR_PIPE_E_DEVICE;
    return drain(p);
}

extern "C" FLDR_PIPE_API void fldr_pipe_destroy(fldr_pipe* p) {
    if (p) close_pipe(p);
}
