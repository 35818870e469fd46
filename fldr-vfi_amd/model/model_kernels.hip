// The two kernels of libfldr_model.so: the 8-bit pixel layout C callers have (interleaved rows with a pitch, BGR or RGB) on either
// side of the forward.  Everything in between runs on the kernels of libfldr_hip.so (model_host.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "model_internal.h"

namespace fldr_model_impl {

// ---- (a) two interleaved 8-bit frames -> every pyramid level in one launch ------------------------------------------------------
// The tiling of ingest_pyramid_kernel (csrc/ingest_kernels.hip): one 64 x 64 tile (+ halo) of one level-0 plane staged in LDS,
// normalised and reflect-padded on the way in, written out as level 0 and reduced to the tile's pixels of every other level.  Only
// the load differs: plane (c, t) is byte c (BGR) or 2 - c (RGB) of the 3-byte pixels of frame t, rows `pitch` bytes apart.  Same
// expressions and operation order as that kernel, hence the same bits as fldr_ingest_pyramid_u8 on the planar rearrangement.
#define MI_T 64
#define MI_LW 72
#define MI_LH 66
struct MiArgs {
    const uint8_t* frame[2];
    int64_t pitch[2];
    float* lv[MI_MAX_LEVELS];
    int n_levels, H, W, Hp, Wp, rgb;
};

__device__ __forceinline__ float mi_norm(uint8_t v) {
#pragma clang fp contract(off)
    float f = (float)v / 255.0f;
    f = f * 2.0f;
    return f - 1.0f;
}

__global__ __launch_bounds__(256) void ingest_interleaved_pyramid_kernel(MiArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float tile[MI_LH * MI_LW];
    const int tid = threadIdx.x;
    const int X0 = blockIdx.x * MI_T, Y0 = blockIdx.y * MI_T;
    const int bct = blockIdx.z;                                          // (c*2 + t) in the output (batch 1)
    const int t = bct & 1, c = bct >> 1;
    const uint8_t* src = a.frame[t] + (a.rgb ? 2 - c : c);
    const int64_t pitch = a.pitch[t];
    for (int e = tid; e < MI_LH * (MI_LW / 4); e += 256) {
        const int r = e / (MI_LW / 4), q = e - r * (MI_LW / 4);
        const int yc = min(max(Y0 - 1 + r, 0), a.Hp - 1);
        const int sy = yc < a.H ? yc : 2 * (a.H - 1) - yc;
        const int x = X0 - 4 + 4 * q;
        float f[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int xc = min(max(x + k, 0), a.Wp - 1);
            const int sx = xc < a.W ? xc : 2 * (a.W - 1) - xc;
            f[k] = mi_norm(src[(int64_t)sy * pitch + 3 * (int64_t)sx]);
        }
        *reinterpret_cast<float4*>(tile + r * MI_LW + 4 * q) = make_float4(f[0], f[1], f[2], f[3]);
    }
    __syncthreads();
    {
        float* out = a.lv[0] + (int64_t)bct * a.Hp * a.Wp;
        for (int e = tid; e < MI_T * (MI_T / 4); e += 256) {
            const int r = e / (MI_T / 4), q = e - r * (MI_T / 4);
            const int y = Y0 + r, x = X0 + 4 * q;
            if (y < a.Hp && x < a.Wp)                                    // (Wp % 4 == 0: host-checked)
                *reinterpret_cast<float4*>(out + (int64_t)y * a.Wp + x) = *reinterpret_cast<const float4*>(tile + (r + 1) * MI_LW + 4 + 4 * q);
        }
    }
    const float c0 = -0.09375f, c1 = 0.59375f;
    for (int l = 1; l < a.n_levels; ++l) {
        const int s = 1 << l, n = MI_T >> l;
        const int Hd = a.Hp >> l, Wd = a.Wp >> l;
        float* out = a.lv[l] + (int64_t)bct * Hd * Wd;
        for (int e = tid; e < n * n; e += 256) {
            const int oy = e / n, ox = e - oy * n;
            const int gy = (Y0 >> l) + oy, gx = (X0 >> l) + ox;
            if (gy >= Hd || gx >= Wd) continue;
            const int lr = oy * s + s / 2 - 1, lc = ox * s + s / 2 + 2;
            float r[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float* row = tile + (lr + j) * MI_LW + lc;
                r[j] = ((row[0] * c0 + row[1] * c1) + row[2] * c1) + row[3] * c0;
            }
            out[(int64_t)gy * Wd + gx] = ((r[0] * c0 + r[1] * c1) + r[2] * c1) + r[3] * c0;
        }
    }
}

int ingest_interleaved_pyramid(const uint8_t* const frame[2], const int64_t pitch[2], int rgb, float* const* levels, int n_levels,
                               int H, int W, int Hp, int Wp, hipStream_t stream) {
    if (!frame[0] || !frame[1] || !levels || n_levels < 1 || n_levels > MI_MAX_LEVELS || H < 2 || W < 2 || Hp < H || Wp < W)
        return FLDR_MODEL_E_ARG;
    if (pitch[0] < 3ll * W || pitch[1] < 3ll * W) return FLDR_MODEL_E_ARG;
    if (Hp - H >= H || Wp - W >= W) return FLDR_MODEL_E_SHAPE;
    if ((Wp & 3) || (Hp & ((1 << (n_levels - 1)) - 1)) || (Wp & ((1 << (n_levels - 1)) - 1))) return FLDR_MODEL_E_SHAPE;
    MiArgs a;
    a.frame[0] = frame[0]; a.frame[1] = frame[1]; a.pitch[0] = pitch[0]; a.pitch[1] = pitch[1];
    a.n_levels = n_levels; a.H = H; a.W = W; a.Hp = Hp; a.Wp = Wp; a.rgb = rgb ? 1 : 0;
    for (int i = 0; i < MI_MAX_LEVELS; ++i) {
        a.lv[i] = i < n_levels ? levels[i] : nullptr;
        if (i < n_levels && !levels[i]) return FLDR_MODEL_E_ARG;
    }
    dim3 grid((Wp + MI_T - 1) / MI_T, (Hp + MI_T - 1) / MI_T, 6);
    hipLaunchKernelGGL(ingest_interleaved_pyramid_kernel, grid, dim3(256), 0, stream, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

// ---- (b) planar rounded 8-bit frame [3,H,W] -> interleaved rows with a pitch -----------------------------------------------------
// One thread per pixel: three byte loads (one per plane, coalesced along the row) and the pixel's three bytes.
__global__ __launch_bounds__(256) void planar_to_interleaved_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                    int64_t pitch, int H, int W, int rgb) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= W) return;
    const int64_t HW = (int64_t)H * W, i = (int64_t)y * W + x;
    const uint8_t p0 = src[i], p1 = src[HW + i], p2 = src[2 * HW + i];
    uint8_t* d = dst + (int64_t)y * pitch + 3 * (int64_t)x;
    d[0] = rgb ? p2 : p0;
    d[1] = p1;
    d[2] = rgb ? p0 : p2;
}

int planar_to_interleaved(const uint8_t* src, uint8_t* dst, int64_t pitch, int rgb, int H, int W, hipStream_t stream) {
    if (!src || !dst || H < 1 || W < 1) return FLDR_MODEL_E_ARG;
    if (pitch < 3ll * W) return FLDR_MODEL_E_ARG;
    hipLaunchKernelGGL(planar_to_interleaved_kernel, dim3((W + 255) / 256, H), dim3(256), 0, stream, src, dst, pitch, H, W, rgb ? 1 : 0);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

}  // namespace fldr_model_impl
