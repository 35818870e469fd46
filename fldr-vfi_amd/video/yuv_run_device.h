// Runs of YUV / BGR samples along a row, device side, inlined into each converter kernel that uses them: the constants of a sample type
// (Smp), values packed into dwords (pack2b, pack2h, pack4) and taken out of them (unpack), one wide access per lane (ld_wide, st_wide), a
// run of sample groups read or written either that way or sample by sample (load_run, store_run), the same for a row of one dword per
// pixel (load_words, store_words), and a 16-bit container word <-> its 10-bit code value (dec, enc).  Then, host side, how such a
// kernel is launched: the alignment predicate of the wide form (al), the grid of a kernel whose threads own runs along rows (row_grid),
// the launch of the VEC or the !VEC instance (YUV_LAUNCH_VEC) and its error as a code (launched).  Included by video_kernels.hip
// (4:2:0; ../light compiles that file again), ../chroma/chroma_kernels.hip (4:2:2, 4:4:4), ../pack10/pack10_kernels.hip (v210, Y210,
// Y410) and ../rgb/rgb_kernels.hip (RGB, alpha).  Which samples a lane owns, the taps and the colour arithmetic stay with the including
// kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fldr_yuv_run {

// chroma centre and largest code value of a sample type: bytes at depth 8, 16-bit words at depth 10
template <typename T> struct Smp;
template <> struct Smp<uint8_t> { static constexpr int MID = 128, MAXV = 255; };
template <> struct Smp<uint16_t> { static constexpr int MID = 512, MAXV = 1023; };

// Values that fit a sample -> one dword (a lowest), through v_perm_b32, never shifts and ORs.  Packed with shifts and ORs, hipcc turns a
// kernel's "clamp (x >> 19), pack two" into v_ashr_pk_u8_i32 (bytes) or v_ashr_pk_* / v_cvt_pk_u16_* (halves) and ORs its result with
// the upper part, which assumes the instruction clears bits 16..31; on gfx950 pixels 2 and 3 of every dword then came out ORed with
// stale bits (measured).  Both libraries are checked for these instructions (tests/test_video_cpu.py, tests/test_video10_cpu.py,
// tests/test_chroma_cpu.py).
__device__ __forceinline__ uint32_t pack2b(int a, int b) { return __builtin_amdgcn_perm((uint32_t)b, (uint32_t)a, 0x0c0c0400u); }   // bytes: a, b, 0, 0
__device__ __forceinline__ uint32_t pack2h(int a, int b) { return __builtin_amdgcn_perm((uint32_t)b, (uint32_t)a, 0x05040100u); }   // halves: a, b
__device__ __forceinline__ uint32_t pack4(int a, int b, int c, int d) { return pack2h((int)pack2b(a, b), (int)pack2b(c, d)); }     // bytes: a, b, c, d

// NB (2, 4, 8, 16 or 32) bytes at an address aligned to min(NB, 16), as dwords (2 bytes: the low half of w[0])
template <int NB>
__device__ __forceinline__ void ld_wide(const uint8_t* p, uint32_t* w) {
    if (NB == 2) {
        w[0] = *reinterpret_cast<const uint16_t*>(p);
    } else if (NB == 4) {
        w[0] = *reinterpret_cast<const uint32_t*>(p);
    } else if (NB == 8) {
        const uint2 v = *reinterpret_cast<const uint2*>(p);
        w[0] = v.x; w[1] = v.y;
    } else {
#pragma unroll
        for (int i = 0; i < NB / 16; ++i) {
            const uint4 v = reinterpret_cast<const uint4*>(p)[i];
            w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
        }
    }
}
template <int NB>
__device__ __forceinline__ void st_wide(uint8_t* p, const uint32_t* w) {
    if (NB == 2) {
        *reinterpret_cast<uint16_t*>(p) = (uint16_t)w[0];
    } else if (NB == 4) {
        *reinterpret_cast<uint32_t*>(p) = w[0];
    } else if (NB == 8) {
        *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
    } else {
#pragma unroll
        for (int i = 0; i < NB / 16; ++i) reinterpret_cast<uint4*>(p)[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
    }
}

// the NS samples that dwords hold, lowest first: s[NS]
template <typename T, int NS>
__device__ __forceinline__ void unpack(const uint32_t* w, int* s) {
#pragma unroll
    for (int e = 0; e < NS; ++e)
        s[e] = sizeof(T) == 1 ? (int)((w[e >> 2] >> (8 * (e & 3))) & 0xffu) : (int)((w[e >> 1] >> (16 * (e & 1))) & 0xffffu);
}

// N groups of G samples each (G = 1: a plane of single samples; 2: interleaved U, V; 4: a packed 4:2:2 group) from group g0 of `row`:
// the raw words, s[N * G].  !VEC: group indices clamped to lim - 1.
template <typename T, int N, int G, bool VEC>
__device__ __forceinline__ void load_run(const uint8_t* row, int g0, int lim, int* s) {
    if (VEC) {
        constexpr int NB = N * G * (int)sizeof(T);
        uint32_t w[(NB + 3) / 4];
        ld_wide<NB>(row + (int64_t)g0 * G * (int)sizeof(T), w);
        unpack<T, N * G>(w, s);
    } else {
        const T* r = reinterpret_cast<const T*>(row);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int gi = min(g0 + j, lim - 1);
#pragma unroll
            for (int q = 0; q < G; ++q) s[j * G + q] = r[gi * G + q];
        }
    }
}

// The inverse: s[N * G] (values that fit a sample) to groups g0 .. g0 + N - 1; !VEC: only groups below lim are written.
template <typename T, int N, int G, bool VEC>
__device__ __forceinline__ void store_run(uint8_t* row, int g0, int lim, const int* s) {
    if (VEC) {
        constexpr int NB = N * G * (int)sizeof(T);
        uint32_t w[(NB + 3) / 4];
        if (NB == 2) {
            w[0] = pack2b(s[0], s[1]);
        } else {
#pragma unroll
            for (int i = 0; i < NB / 4; ++i)
                w[i] = sizeof(T) == 1 ? pack4(s[4 * i], s[4 * i + 1], s[4 * i + 2], s[4 * i + 3]) : pack2h(s[2 * i], s[2 * i + 1]);
        }
        st_wide<NB>(row + (int64_t)g0 * G * (int)sizeof(T), w);
    } else {
        T* r = reinterpret_cast<T*>(row);
#pragma unroll
        for (int j = 0; j < N; ++j)
            if (g0 + j < lim) {
#pragma unroll
                for (int q = 0; q < G; ++q) r[(g0 + j) * G + q] = (T)s[j * G + q];
            }
    }
}

// N pixel dwords (one per pixel: Y410, the RGB word layouts) from pixel x0 of `row`: w[N].  !VEC: pixel indices clamped to lim - 1.
// The four word kernels of ../pack10 and ../rgb call the VEC forms only and keep their per-sample loops in the kernel: written through
// these helpers, hipcc gave those kernels other code than before (DESIGN_LOG.md); the alpha kernels take both forms from here.
template <int N, bool VEC>
__device__ __forceinline__ void load_words(const uint8_t* row, int x0, int lim, uint32_t* w) {
    if (VEC) {
        ld_wide<4 * N>(row + (int64_t)x0 * 4, w);
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) w[j] = reinterpret_cast<const uint32_t*>(row)[min(x0 + j, lim - 1)];
    }
}

// The inverse: w[N] to pixels x0 .. x0 + N - 1; !VEC: only pixels below lim are written.
template <int N, bool VEC>
__device__ __forceinline__ void store_words(uint8_t* row, int x0, int lim, const uint32_t* w) {
    if (VEC) {
        st_wide<4 * N>(row + (int64_t)x0 * 4, w);
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j)
            if (x0 + j < lim) reinterpret_cast<uint32_t*>(row)[x0 + j] = w[j];
    }
}

// container word <-> code value: bytes are the value; 16-bit words keep it in the high 10 bits (HIGH: NV12 at depth 10 = P010, semiplanar
// P210 / P410) or in the low 10
template <typename T, bool HIGH>
__device__ __forceinline__ int dec(int w) { return sizeof(T) == 1 ? w : HIGH ? (w >> 6) : (w & 0x3ff); }
template <typename T, bool HIGH>
__device__ __forceinline__ int enc(int v) { return sizeof(T) == 2 && HIGH ? v << 6 : v; }

// ---- host side: launching a converter kernel ---------------------------------------------------------------------------------------
// is a pointer or a pitch a multiple of n (a power of two)?
template <typename V> static bool al(V v, uintptr_t n) { return ((uintptr_t)v & (n - 1)) == 0; }

// the grid of a kernel whose TX x TY blocks own `run` pixels per thread along each of H rows, n frames (or planes) deep
template <int TX, int TY> static dim3 row_grid(int run, int H, int W, int n) {
    return dim3(((W + run - 1) / run + TX - 1) / TX, (H + TY - 1) / TY, n);
}

// KERNEL<..., vec><<<grid, block, 0, stream>>>(a); the arguments after `a` are KERNEL's template arguments in front of VEC
#define YUV_LAUNCH_VEC(KERNEL, vec, grid, block, stream, a, ...)                                   \
    do {                                                                                           \
        if (vec) hipLaunchKernelGGL((KERNEL<__VA_ARGS__, true>), grid, block, 0, stream, a);       \
        else hipLaunchKernelGGL((KERNEL<__VA_ARGS__, false>), grid, block, 0, stream, a);          \
    } while (0)

// the error of the launches since the last call, as a return code
static int launched() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

}  // namespace fldr_yuv_run
