// The kernels of libfldr_rgb.so: the four-byte layouts (BGRA, RGBA, ARGB, ABGR), the two 10-bit words (X2RGB10, X2BGR10) and planar
// GBR(A) at 8 or 10 bits on either side of the model's planar BGR forward, and the alpha pass.  All are bandwidth kernels without
// arithmetic on colour: a code value is moved, never changed.
//   word layouts <-> planar BGR   one input and one output kernel, templated on the layout (which gives the sample type: uint8 for
//            the byte layouts, uint16 for the 10-bit words).  A thread owns RUN_WORDS = 4 pixels along one row: 16 bytes of the frame
//            and one dword (uint8) or one uint2 (uint16) of each BGR plane, so the lanes of a wave touch 1024 contiguous bytes of the
//            frame and 256 / 512 contiguous bytes of each plane per instruction.
//            VEC    the frame's plane and pitch are 16-byte aligned, W % 4 == 0 and the planar frame is 4- (uint8) / 8-byte (uint16)
//                   aligned: every planar row then starts on a whole access;
//            !VEC   the same shuffling on single words, indices clamped into the row and the stores guarded.
//   GBRP / GBRAP <-> planar BGR   a plane permutation: one row-copy kernel templated on the sample type; a thread owns 16 bytes of a
//            row of one plane (blockIdx.z walks the planes), masks 16-bit samples with 0x3ff, and fills a plane that has no source
//            (the A plane of an output frame) with the largest code.  VEC: every plane, pitch and row length a multiple of 16 bytes.
//   alpha    grid (row walkers, outputs): block x walks rows, its threads walk groups of four pixels, blockIdx.y is the output k whose
//            time t[k] is read here.  Templated on where alpha lives on either side (a field of a 32-bit pixel word, a byte plane, a
//            16-bit plane); NEARER reads the chosen input, BLEND both; only the alpha field (a read-modify-write of the pixel words)
//            or the A plane of the output is written.  VEC: four pixels per access on every side.
// The dwords of the byte layouts and of the planar rows are built with v_perm_b32 (pack4 / pack2h of ../video/yuv_run_device.h), the
// 10-bit words as whole dwords a | b << 10 | c << 20: never half-word shift-and-OR packing, so none of the instructions that header
// warns of can appear.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <type_traits>

#include "../video/yuv_run_device.h"
#include "rgb_internal.h"

namespace fldr_rgb_impl {

#define RG_TX 64                 // threads along a row
#define RG_TY 4                  // rows per block
#define RG_ALPHA_THREADS 256     // threads of an alpha block (one row at a time)
#define RG_ALPHA_BLOCKS 2048     // row walkers at most

using namespace fldr_yuv_run;                      // Smp, ld_wide / st_wide, load_run / store_run, load_words / store_words, pack2h, pack4, unpack;
                                                   // al, row_grid, YUV_LAUNCH_VEC, launched

// Where the channels sit in a pixel word (bit offsets), the bits of a colour field and the planar sample type.
template <int L> struct Lay;
template <> struct Lay<FLDR_RGB_BGRA> { typedef uint8_t T; static constexpr int SB = 0, SG = 8, SR = 16, SA = 24, BITS = 8; };
template <> struct Lay<FLDR_RGB_RGBA> { typedef uint8_t T; static constexpr int SB = 16, SG = 8, SR = 0, SA = 24, BITS = 8; };
template <> struct Lay<FLDR_RGB_ARGB> { typedef uint8_t T; static constexpr int SB = 24, SG = 16, SR = 8, SA = 0, BITS = 8; };
template <> struct Lay<FLDR_RGB_ABGR> { typedef uint8_t T; static constexpr int SB = 8, SG = 16, SR = 24, SA = 0, BITS = 8; };
template <> struct Lay<FLDR_RGB_X2RGB10> { typedef uint16_t T; static constexpr int SB = 0, SG = 10, SR = 20, SA = 30, BITS = 10; };
template <> struct Lay<FLDR_RGB_X2BGR10> { typedef uint16_t T; static constexpr int SB = 20, SG = 10, SR = 0, SA = 30, BITS = 10; };

// one pixel word with opaque alpha from three values that fit their fields
template <int L> __device__ __forceinline__ uint32_t pixel_word(int b, int g, int r) {
    if constexpr (L == FLDR_RGB_BGRA) return pack4(b, g, r, 255);
    else if constexpr (L == FLDR_RGB_RGBA) return pack4(r, g, b, 255);
    else if constexpr (L == FLDR_RGB_ARGB) return pack4(255, r, g, b);
    else if constexpr (L == FLDR_RGB_ABGR) return pack4(255, b, g, r);
    else return ((uint32_t)b << Lay<L>::SB) | ((uint32_t)g << Lay<L>::SG) | ((uint32_t)r << Lay<L>::SR) | 0xc0000000u;
}

// ---- (a) word layouts -> planar BGR ------------------------------------------------------------------------------------------------
struct InArgs {
    const uint8_t* plane[MAX_FRAMES];
    int64_t pitch[MAX_FRAMES];       // bytes
    uint8_t* dst;                    // [n][3][H][W] of T
    int H, W;
};

template <int L, bool VEC>
__global__ __launch_bounds__(RG_TX * RG_TY) void rgb_words_to_planar_kernel(InArgs a) {
    typedef typename Lay<L>::T T;
    constexpr int R = RUN_WORDS;
    constexpr uint32_t M = (1u << Lay<L>::BITS) - 1u;
    const int x0 = R * (blockIdx.x * RG_TX + threadIdx.x);
    const int y = blockIdx.y * RG_TY + threadIdx.y;
    const int f = blockIdx.z;
    const int H = a.H, W = a.W;
    if (x0 >= W || y >= H) return;
    const uint8_t* row0 = a.plane[f] + (int64_t)y * a.pitch[f];
    uint32_t w[R];
    if (VEC) {
        load_words<R, true>(row0, x0, W, w);
    } else {                                         // in the kernel: DESIGN_LOG.md ("Chroma, pack10 and rgb", device code)
#pragma unroll
        for (int j = 0; j < R; ++j) w[j] = reinterpret_cast<const uint32_t*>(row0)[min(x0 + j, W - 1)];
    }
    int bb[R], gg[R], rr[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        bb[j] = (int)((w[j] >> Lay<L>::SB) & M);
        gg[j] = (int)((w[j] >> Lay<L>::SG) & M);
        rr[j] = (int)((w[j] >> Lay<L>::SR) & M);
    }
    const int64_t HW = (int64_t)H * W;
    const int64_t plane_bytes = HW * (int64_t)sizeof(T);
    uint8_t* d = a.dst + ((int64_t)f * 3 * HW + (int64_t)y * W) * (int64_t)sizeof(T);
    store_run<T, R, 1, VEC>(d, x0, W, bb);
    store_run<T, R, 1, VEC>(d + plane_bytes, x0, W, gg);
    store_run<T, R, 1, VEC>(d + 2 * plane_bytes, x0, W, rr);
}

// ---- (b) planar BGR frame -> word layouts -----------------------------------------------------------------------------------------
struct OutArgs {
    const uint8_t* src;              // [3][H][W] of T
    uint8_t* plane;
    int64_t pitch;                   // bytes
    int H, W;
};

template <int L, bool VEC>
__global__ __launch_bounds__(RG_TX * RG_TY) void rgb_words_from_planar_kernel(OutArgs a) {
    typedef typename Lay<L>::T T;
    constexpr int R = RUN_WORDS;
    constexpr int M = (1 << Lay<L>::BITS) - 1;
    const int x0 = R * (blockIdx.x * RG_TX + threadIdx.x);
    const int y = blockIdx.y * RG_TY + threadIdx.y;
    const int H = a.H, W = a.W;
    if (x0 >= W || y >= H) return;
    const int64_t HW = (int64_t)H * W;
    int px[3][R];
#pragma unroll
    for (int c = 0; c < 3; ++c) load_run<T, R, 1, VEC>(a.src + ((int64_t)c * HW + (int64_t)y * W) * (int64_t)sizeof(T), x0, W, px[c]);
    uint32_t w[R];
#pragma unroll
    for (int j = 0; j < R; ++j) w[j] = pixel_word<L>(px[0][j] & M, px[1][j] & M, px[2][j] & M);
    uint8_t* row0 = a.plane + (int64_t)y * a.pitch;
    if (VEC) {
        store_words<R, true>(row0, x0, W, w);
    } else {                                         // in the kernel, like the input kernel's loads
#pragma unroll
        for (int j = 0; j < R; ++j)
            if (x0 + j < W) reinterpret_cast<uint32_t*>(row0)[x0 + j] = w[j];
    }
}

// ---- (c) rows of planes: GBRP / GBRAP <-> planar BGR --------------------------------------------------------------------------------
constexpr int MAX_PLANES = 3 * MAX_FRAMES;           // planes one launch copies (blockIdx.z): two frames in, or G, B, R, A out
struct PlaneArgs {
    const uint8_t* src[MAX_PLANES];  // nullptr: the destination plane is filled with the largest code
    int64_t spitch[MAX_PLANES];      // bytes
    uint8_t* dst[MAX_PLANES];
    int64_t dpitch[MAX_PLANES];
    int H, W;
};

template <typename T, bool VEC>
__global__ __launch_bounds__(RG_TX * RG_TY) void rgb_planes_kernel(PlaneArgs a) {
    constexpr int N = RUN_PLANE_BYTES / (int)sizeof(T);
    constexpr uint32_t MASK = sizeof(T) == 2 ? 0x03ff03ffu : 0xffffffffu;          // dwords of samples; also the largest codes
    const int x0 = N * (blockIdx.x * RG_TX + threadIdx.x);
    const int y = blockIdx.y * RG_TY + threadIdx.y;
    const int z = blockIdx.z;
    const int W = a.W;
    if (x0 >= W || y >= a.H) return;
    const uint8_t* s = a.src[z];                                                   // the same in every lane
    uint8_t* drow = a.dst[z] + (int64_t)y * a.dpitch[z];
    const uint8_t* srow = s ? s + (int64_t)y * a.spitch[z] : nullptr;
    if (VEC) {
        uint32_t w[4] = {MASK, MASK, MASK, MASK};
        if (s) {
            ld_wide<16>(srow + (int64_t)x0 * (int64_t)sizeof(T), w);
#pragma unroll
            for (int i = 0; i < 4; ++i) w[i] &= MASK;
        }
        st_wide<16>(drow + (int64_t)x0 * (int64_t)sizeof(T), w);
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j)
            if (x0 + j < W) reinterpret_cast<T*>(drow)[x0 + j] = s ? (T)(reinterpret_cast<const T*>(srow)[x0 + j] & (T)MASK) : (T)MASK;
    }
}

// ---- (d) alpha ------------------------------------------------------------------------------------------------------------------
enum { AK_WORD = 0,              // a field of a 32-bit pixel word (shift, mask)
       AK_U8 = 1,                // a byte plane
       AK_U16 = 2 };             // a 16-bit plane, value in the low 10 bits

struct AlphaArgs {
    const uint8_t* in[2];
    int64_t in_pitch[2];             // bytes
    uint8_t* out[ALPHA_MAX_OUT];
    int64_t out_pitch[ALPHA_MAX_OUT];
    const float* t;                  // the times of these outputs
    int H, W;
    int blend;                       // 0: NEARER, 1: BLEND
    int in_shift, out_shift;         // AK_WORD: the field's lowest bit
    uint32_t mask;                   // the field's largest code
};

// the alpha of pixels x .. x + 3 of a row (!VEC: indices clamped into the row)
template <int K, bool VEC> __device__ __forceinline__ void load_alpha(const uint8_t* row, int x, int W, int shift, uint32_t mask, uint32_t* al) {
    if constexpr (K == AK_WORD) {
        uint32_t w[4];
        load_words<4, VEC>(row, x, W, w);
#pragma unroll
        for (int j = 0; j < 4; ++j) al[j] = (w[j] >> shift) & mask;
    } else {
        typedef typename std::conditional<K == AK_U8, uint8_t, uint16_t>::type T;
        int s[4];
        load_run<T, 4, 1, VEC>(row, x, W, s);
#pragma unroll
        for (int j = 0; j < 4; ++j) al[j] = (uint32_t)s[j] & mask;
    }
}

// the inverse: only alpha is written (!VEC: only pixels below W)
template <int K, bool VEC> __device__ __forceinline__ void store_alpha(uint8_t* row, int x, int W, int shift, uint32_t mask, const uint32_t* al) {
    if constexpr (K == AK_WORD) {
        const uint32_t keep = ~(mask << shift);
        if (VEC) {
            uint32_t w[4];
            ld_wide<16>(row + (int64_t)x * 4, w);
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = (w[j] & keep) | (al[j] << shift);
            st_wide<16>(row + (int64_t)x * 4, w);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x + j < W) {
                    uint32_t* p = reinterpret_cast<uint32_t*>(row) + x + j;
                    *p = (*p & keep) | (al[j] << shift);
                }
        }
    } else {
        typedef typename std::conditional<K == AK_U8, uint8_t, uint16_t>::type T;
        const int s[4] = {(int)al[0], (int)al[1], (int)al[2], (int)al[3]};
        store_run<T, 4, 1, VEC>(row, x, W, s);
    }
}

template <int SK, int DK, bool VEC>
__global__ __launch_bounds__(RG_ALPHA_THREADS) void rgb_alpha_kernel(AlphaArgs a) {
    const int k = blockIdx.y;
    const float tk = a.t[k];
    const int W = a.W;
    // BLEND: the weight of in[1], 16 fraction bits (NaN fails the comparison: 0).  NEARER: the input read.
    const uint32_t wt = tk >= 0.0f ? (uint32_t)fminf(rintf(tk * 65536.0f), 65536.0f) : 0u;
    const int nearer = tk < 0.5f ? 0 : 1;
    const uint8_t* in_n = nearer ? a.in[1] : a.in[0];
    const int64_t pitch_n = nearer ? a.in_pitch[1] : a.in_pitch[0];
    for (int y = blockIdx.x; y < a.H; y += gridDim.x) {
        uint8_t* orow = a.out[k] + (int64_t)y * a.out_pitch[k];
        for (int x = 4 * threadIdx.x; x < W; x += 4 * RG_ALPHA_THREADS) {
            uint32_t al[4];
            if (a.blend) {
                uint32_t a1[4];
                load_alpha<SK, VEC>(a.in[0] + (int64_t)y * a.in_pitch[0], x, W, a.in_shift, a.mask, al);
                load_alpha<SK, VEC>(a.in[1] + (int64_t)y * a.in_pitch[1], x, W, a.in_shift, a.mask, a1);
#pragma unroll
                for (int j = 0; j < 4; ++j) al[j] = (al[j] * (65536u - wt) + a1[j] * wt + 32768u) >> 16;
            } else {
                load_alpha<SK, VEC>(in_n + (int64_t)y * pitch_n, x, W, a.in_shift, a.mask, al);
            }
            store_alpha<DK, VEC>(orow, x, W, a.out_shift, a.mask, al);
        }
    }
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------

// Call GO(L) for the word layout of `fmt` (the caller checked the format).
#define RG_DISPATCH(fmt)                                                     \
    do {                                                                     \
        switch ((fmt).layout) {                                              \
        case FLDR_RGB_BGRA: GO(FLDR_RGB_BGRA); break;                        \
        case FLDR_RGB_RGBA: GO(FLDR_RGB_RGBA); break;                        \
        case FLDR_RGB_ARGB: GO(FLDR_RGB_ARGB); break;                        \
        case FLDR_RGB_ABGR: GO(FLDR_RGB_ABGR); break;                        \
        case FLDR_RGB_X2RGB10: GO(FLDR_RGB_X2RGB10); break;                  \
        default: GO(FLDR_RGB_X2BGR10); break;                                \
        }                                                                    \
    } while (0)

// model plane c (B, G, R) is plane GBR_OF[c] of a GBRP / GBRAP frame (G, B, R, A)
static const int GBR_OF[3] = {1, 0, 2};

static int launch_planes(const PlaneArgs& a, bool wide16, bool vec, int H, int W, int n, hipStream_t stream) {
    const dim3 block(RG_TX, RG_TY);
    const dim3 grid = row_grid<RG_TX, RG_TY>(RUN_PLANE_BYTES / (wide16 ? 2 : 1), H, W, n);
    if (wide16) YUV_LAUNCH_VEC(rgb_planes_kernel, vec, grid, block, stream, a, uint16_t);
    else YUV_LAUNCH_VEC(rgb_planes_kernel, vec, grid, block, stream, a, uint8_t);
    return launched();
}

int to_planar(const fldr_rgb_frame* in, int n, const fldr_rgb_format& fmt, void* planar, int H, int W, hipStream_t stream) {
    const int sb = words16(fmt) ? 2 : 1;                                           // bytes of a planar sample
    const dim3 block(RG_TX, RG_TY);
    if (!word_layout(fmt)) {
        PlaneArgs a;
        memset(&a, 0, sizeof(a));
        bool vec = al((int64_t)W * sb, 16) && al(planar, 16);
        for (int f = 0; f < n; ++f)
            for (int c = 0; c < 3; ++c) {
                const int z = 3 * f + c, p = GBR_OF[c];
                a.src[z] = (const uint8_t*)in[f].plane[p]; a.spitch[z] = in[f].pitch[p];
                a.dst[z] = (uint8_t*)planar + (int64_t)z * H * W * sb; a.dpitch[z] = (int64_t)W * sb;
                vec = vec && al(in[f].plane[p], 16) && al(in[f].pitch[p], 16);
            }
        a.H = H; a.W = W;
        return launch_planes(a, sb == 2, vec, H, W, 3 * n, stream);
    }
    InArgs a;
    bool vec = W % RUN_WORDS == 0 && al(planar, (uintptr_t)(RUN_WORDS * sb));
    for (int f = 0; f < MAX_FRAMES; ++f) {
        a.plane[f] = f < n ? (const uint8_t*)in[f].plane[0] : nullptr;
        a.pitch[f] = f < n ? in[f].pitch[0] : 0;
        if (f < n) vec = vec && al(in[f].plane[0], 16) && al(in[f].pitch[0], 16);
    }
    a.dst = (uint8_t*)planar; a.H = H; a.W = W;
#define GO(L) YUV_LAUNCH_VEC(rgb_words_to_planar_kernel, vec, (row_grid<RG_TX, RG_TY>(RUN_WORDS, H, W, n)), block, stream, a, L)
    RG_DISPATCH(fmt);
#undef GO
    return launched();
}

int from_planar(const void* planar, const fldr_rgb_frame& out, const fldr_rgb_format& fmt, int H, int W, hipStream_t stream) {
    const int sb = words16(fmt) ? 2 : 1;
    const dim3 block(RG_TX, RG_TY);
    if (!word_layout(fmt)) {
        PlaneArgs a;
        memset(&a, 0, sizeof(a));
        const int np = fmt.layout == FLDR_RGB_GBRAP ? 4 : 3;
        bool vec = al((int64_t)W * sb, 16) && al(planar, 16);
        for (int c = 0; c < 3; ++c) {
            const int z = GBR_OF[c];
            a.src[z] = (const uint8_t*)planar + (int64_t)c * H * W * sb; a.spitch[z] = (int64_t)W * sb;
        }
        for (int z = 0; z < np; ++z) {                                             // z = 3: no source, the A plane becomes opaque
            a.dst[z] = (uint8_t*)out.plane[z]; a.dpitch[z] = out.pitch[z];
            vec = vec && al(out.plane[z], 16) && al(out.pitch[z], 16);
        }
        a.H = H; a.W = W;
        return launch_planes(a, sb == 2, vec, H, W, np, stream);
    }
    OutArgs a;
    const bool vec = W % RUN_WORDS == 0 && al(planar, (uintptr_t)(RUN_WORDS * sb)) && al(out.plane[0], 16) && al(out.pitch[0], 16);
    a.src = (const uint8_t*)planar; a.plane = (uint8_t*)out.plane[0]; a.pitch = out.pitch[0]; a.H = H; a.W = W;
#define GO(L) YUV_LAUNCH_VEC(rgb_words_from_planar_kernel, vec, (row_grid<RG_TX, RG_TY>(RUN_WORDS, H, W, 1)), block, stream, a, L)
    RG_DISPATCH(fmt);
#undef GO
    return launched();
}

// where a format keeps alpha: the kind, the plane, the field's lowest bit, and the alignment four pixels of it need
struct AlphaPlace { int kind, plane, shift; uintptr_t unit; };
static AlphaPlace alpha_place(const fldr_rgb_format& f) {
    if (f.layout <= FLDR_RGB_ABGR) return {AK_WORD, 0, f.layout <= FLDR_RGB_RGBA ? 24 : 0, 16};
    if (f.layout <= FLDR_RGB_X2BGR10) return {AK_WORD, 0, 30, 16};
    return words16(f) ? AlphaPlace{AK_U16, 3, 0, 8} : AlphaPlace{AK_U8, 3, 0, 4};
}

int write_alpha(const fldr_rgb_frame in[2], const fldr_rgb_format& fin, const fldr_rgb_frame* out, int n, const fldr_rgb_format& fout,
                const float* t, int H, int W, hipStream_t stream) {
    const AlphaPlace pi = alpha_place(fin), po = alpha_place(fout);
    AlphaArgs a;
    memset(&a, 0, sizeof(a));
    bool vec = W % 4 == 0;
    for (int f = 0; f < 2; ++f) {
        a.in[f] = (const uint8_t*)in[f].plane[pi.plane]; a.in_pitch[f] = in[f].pitch[pi.plane];
        vec = vec && al(a.in[f], pi.unit) && al(a.in_pitch[f], pi.unit);
    }
    for (int k = 0; k < n; ++k) {
        a.out[k] = (uint8_t*)out[k].plane[po.plane]; a.out_pitch[k] = out[k].pitch[po.plane];
        vec = vec && al(a.out[k], po.unit) && al(a.out_pitch[k], po.unit);
    }
    a.t = t; a.H = H; a.W = W;
    a.blend = fout.alpha == FLDR_RGB_ALPHA_BLEND;
    a.in_shift = pi.shift; a.out_shift = po.shift;
    a.mask = (1u << alpha_bits(fout)) - 1u;
    const dim3 grid((unsigned)(H < RG_ALPHA_BLOCKS ? H : RG_ALPHA_BLOCKS), (unsigned)n);
#define GO(SK, DK) YUV_LAUNCH_VEC(rgb_alpha_kernel, vec, grid, dim3(RG_ALPHA_THREADS), stream, a, SK, DK)
    // alpha of one width on both sides (the caller checked): a 16-bit plane only meets a 16-bit plane
    if (pi.kind == AK_U16) GO(AK_U16, AK_U16);
    else if (pi.kind == AK_WORD && po.kind == AK_WORD) GO(AK_WORD, AK_WORD);
    else if (pi.kind == AK_WORD) GO(AK_WORD, AK_U8);
    else if (po.kind == AK_WORD) GO(AK_U8, AK_WORD);
    else GO(AK_U8, AK_U8);
#undef GO
    return launched();
}

}  // namespace fldr_rgb_impl
