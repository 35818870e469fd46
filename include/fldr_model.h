/*
 * fldr_model.h — C model API of libfldr_model.so: the whole fLDRnet frame-pair interpolation (DCTXVFInet.forward with
 * every switch at its default) behind one create / forward pair, for callers that do not embed Python or torch
 * (video players, filters, serving processes).
 *
 * Plain C99; no HIP header is needed: the stream is a void* (a hipStream_t, as fldr_stream_t of fldr_hip.h).  The library
 * drives the public kernels of libfldr_hip.so (include/fldr_hip.h) and nothing else of it.
 *
 * Contract ("C model API"):
 *   - fldr_model_create* uploads the weights, runs every weight prepack, reads T_param / z_alpha on the host and binds the
 *     device's status block (fldr_status_word).  It allocates and synchronises; the model is read-only afterwards.
 *   - fldr_model_forward enqueues one forward on `stream`: no allocation, no synchronisation, no host<->device copy, so it can
 *     be captured into a graph.  All scratch lives in the caller's workspace (fldr_model_workspace_bytes).  Forwards on
 *     different streams with different workspaces may run concurrently on one model.
 *   - The call makes the model's device current and restores the caller's device before it returns.
 *   - On entry it reads the device's two status words (no synchronisation); if a kernel of an earlier call stored a fault flag
 *     it returns FLDR_MODEL_E_STATUS and enqueues nothing.
 *   - One frame pair per call (batch 1): the PCA min / max of the model is taken over the whole batch, so a batch is not a set
 *     of independent pairs.
 * Every function returns 0 or a negative FLDR_MODEL_E_* code, or a positive hipError_t from the runtime.
 */
#ifndef FLDR_MODEL_H
#define FLDR_MODEL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FLDR_MODEL_VERSION 101           /* major*10000 + minor*100 + patch of this header; 101: the 10-bit forms (IN / OUT_U10_PLANAR) */

#define FLDR_MODEL_E_ARG        (-1)     /* bad argument: null pointer, non-positive size, unknown enum value, bad pitch */
#define FLDR_MODEL_E_SHAPE      (-2)     /* frame size the model cannot take (reflect padding needs pad < size) */
#define FLDR_MODEL_E_STATUS     (-3)     /* a device fault flag is set (fldr_status_word), or the status block could not be bound */
#define FLDR_MODEL_E_WORKSPACE  (-10)    /* workspace smaller than fldr_model_workspace_bytes */
#define FLDR_MODEL_E_BATCH      (-11)    /* batch != 1 */
#define FLDR_MODEL_E_IO         (-12)    /* file cannot be opened or read */
#define FLDR_MODEL_E_FORMAT     (-13)    /* not an uncompressed zip of .npy files / malformed .npy header */
#define FLDR_MODEL_E_COMPRESSED (-14)    /* a zip entry is compressed (np.savez_compressed): only stored entries are read */
#define FLDR_MODEL_E_TRUNCATED  (-15)    /* the file ends inside a record or an entry's data */
#define FLDR_MODEL_E_MISSING    (-16)    /* a tensor the forward reads is absent */
#define FLDR_MODEL_E_TENSOR_SHAPE (-17)  /* a tensor has the wrong shape */
#define FLDR_MODEL_E_DTYPE      (-18)    /* a tensor has the wrong dtype (or is not little-endian C order) */
#define FLDR_MODEL_E_DEVICE     (-19)    /* no such device / allocation failed */

#define FLDR_MODEL_API __attribute__((visibility("default")))

typedef struct fldr_model fldr_model;

enum { FLDR_MODEL_F32 = 0, FLDR_MODEL_F64 = 1 };

/* One state-dict tensor in host memory, C-contiguous.  Names as in DCTXVFInet.state_dict() (either alias: "vfinet.conv_flow1.weight"
 * or "base_modules.1.conv_flow1.weight"); the conv weights / biases are fp32, EV8 / Mean8 / meanVec8 / T_param / z_alpha fp64. */
typedef struct fldr_model_tensor {
    const char* name;
    const void* data;
    int32_t     dtype;                   /* FLDR_MODEL_F32 / FLDR_MODEL_F64 */
    int32_t     ndim;                    /* 1 .. 4 */
    int64_t     shape[4];
} fldr_model_tensor;

typedef struct fldr_model_config {
    int32_t device;                      /* HIP device ordinal */
    int32_t test_scales;                 /* pyramid depth S_tst, 3 .. 7 (S_tst + 1 levels); 0 = 5, the shipped configuration */
    int32_t reserved[6];                 /* zero */
} fldr_model_config;

enum { FLDR_MODEL_IN_PYRAMID = 0,        /* pyramid[i]: fp32 [1,3,2,Hp>>i,Wp>>i], i <= S_tst (normInput of DCTXVFInet.forward) */
       FLDR_MODEL_IN_U8_PLANAR = 1,      /* frames_u8: [1,2,3,H,W] uint8 (I0, I1), as fldr_harness.interpolate_u8 takes them */
       FLDR_MODEL_IN_U8_INTERLEAVED = 2, /* frame[0] = I0, frame[1] = I1: H rows of W 3-byte pixels, frame_pitch bytes apart */
       FLDR_MODEL_IN_U10_PLANAR = 3      /* frames_u8 points at [1,2,3,H,W] uint16 (2-byte aligned), 10-bit code values 0 .. 1023 normalised as
                                            v / 1023 * 2 - 1; a value above 1023 is the caller's error and is read as 1023 */ };
enum { FLDR_MODEL_OUT_F64 = 0,           /* out[k]: fp64 [1,3,Hp,Wp], the frame before DCTXVFInet.forward's crop view */
       FLDR_MODEL_OUT_U8_PLANAR = 1,     /* out[k]: uint8 [1,3,H,W], cropped and rounded (np.around of the de-normalised frame) */
       FLDR_MODEL_OUT_U8_INTERLEAVED = 2,/* out[k]: H rows of W 3-byte pixels, out_pitch bytes apart */
       FLDR_MODEL_OUT_U10_PLANAR = 3     /* out[k]: uint16 [1,3,H,W] (4-byte aligned), cropped and rounded to 10-bit code values:
                                            rint(clip((x + 1) / 2, 0, 1) * 1023), half to even.  Any input form goes with any output form */ };
enum { FLDR_MODEL_BGR = 0, FLDR_MODEL_RGB = 1 };   /* channel order of interleaved frames; plane c of the model = BGR channel c */

#define FLDR_MODEL_MAX_LEVELS 8

/* Inputs and outputs of one forward.  Hp, Wp = H, W rounded up to a multiple of 2^S_tst * 8.  All pointers are device pointers
 * except `out` itself (a host array of n_t device pointers, read during the call). */
typedef struct fldr_model_io {
    int32_t        batch;                /* must be 1 */
    int32_t        H, W;                 /* frame size */
    int32_t        input;                /* FLDR_MODEL_IN_* */
    const float*   pyramid[FLDR_MODEL_MAX_LEVELS];   /* IN_PYRAMID: the input; 8-bit inputs: NULL, or where the ingested levels are
                                                        written (instead of the workspace) for a caller that keeps them */
    const uint8_t* frames_u8;            /* IN_U8_PLANAR; IN_U10_PLANAR: the uint16 frames through this pointer */
    const uint8_t* frame[2];
    int64_t        frame_pitch[2];       /* >= 3 W */
    int32_t        in_order;             /* FLDR_MODEL_BGR / FLDR_MODEL_RGB */
    int32_t        n_t;                  /* outputs: >= 1 */
    const float*   t;                    /* n_t floats on the device (output k at t[k]); may be rewritten between graph replays */
    int32_t        output;               /* FLDR_MODEL_OUT_* */
    int32_t        out_order;            /* FLDR_MODEL_BGR / FLDR_MODEL_RGB */
    void* const*   out;                  /* n_t device pointers */
    int64_t        out_pitch;            /* FLDR_MODEL_OUT_U8_INTERLEAVED: >= 3 W */
} fldr_model_io;

FLDR_MODEL_API int         fldr_model_version(void);
FLDR_MODEL_API const char* fldr_model_error_string(int code);
/* 0: sizeof(fldr_model_tensor), 1: fldr_model_config, 2: fldr_model_io — binding self-check; FLDR_MODEL_E_ARG otherwise */
FLDR_MODEL_API int         fldr_model_sizeof(int which);

FLDR_MODEL_API int  fldr_model_create(const fldr_model_tensor* tensors, int n, const fldr_model_config* cfg, fldr_model** out);
/* The shipped weights file (fldr-vfi_amd/weights/, a .npz: an uncompressed zip of .npy files).  Every malformed input is rejected
 * with its code before any HIP call. */
FLDR_MODEL_API int  fldr_model_create_npz(const char* path, const fldr_model_config* cfg, fldr_model** out);
FLDR_MODEL_API void fldr_model_destroy(fldr_model* model);

/* Bytes of workspace one forward of an H x W pair with n_t outputs needs (any input / output form); negative on bad sizes. */
FLDR_MODEL_API int64_t fldr_model_workspace_bytes(const fldr_model* model, int H, int W, int n_t);
/* Enqueue one forward on `stream` (NULL = the null stream).  ws: device memory of at least ws_bytes >= fldr_model_workspace_bytes,
 * 256-byte aligned; it must not be used by another forward in flight. */
FLDR_MODEL_API int fldr_model_forward(const fldr_model* model, const fldr_model_io* io, void* ws, int64_t ws_bytes, void* stream);

/* Synchronous convenience: two interleaved 8-bit host frames (H rows of W 3-byte pixels, pitch bytes apart, channel order `order`)
 * in, n_t interleaved 8-bit host frames (same geometry) out, at t[0 .. n_t-1].  Allocates, uploads, runs, downloads, frees. */
FLDR_MODEL_API int fldr_model_interpolate_host(const fldr_model* model, const uint8_t* i0, const uint8_t* i1, int H, int W, int64_t pitch,
                                               int order, const float* t, int n_t, uint8_t* const* out);

#ifdef __cplusplus
}
#endif
#endif /* FLDR_MODEL_H */
