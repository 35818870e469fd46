// libfldr_model.so, host side: the default fLDRnet forward (DCTXVFInet.forward with no FLDR_* variable set, fLDRnet.py and the
// fldr_hip.py wrappers it calls) as a sequence of calls into the public C ABI of libfldr_hip.so — nothing else of that library is
// used.  Weights and their prepacks live in one device allocation made at create; every buffer of a forward is a slice of the
// caller's workspace, so a forward allocates nothing, synchronises nothing and copies nothing between host and device.
//
// The split-packed ("Spk") views of fldr_hip.py (narrow, sample, channel_halves) are pointer arithmetic here: a packed tensor of C
// channels is ceil(C/8) groups of 2 * H * W * 16 bytes, samples fldr_spk_bytes(C, H, W) apart.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fldr_hip.h"
#include "model_internal.h"

using namespace fldr_model_impl;

namespace {

constexpr int K_PCA = 16;          // components of the 8x8 block projection: int(64 * 1/4) (fldr_harness.prepare_model)
constexpr int NCH = 96;            // dctvfi_nf (16) * img_ch (3) * 2: feature channels per pyramid level
constexpr int HALF = 48;
constexpr int64_t ALIGN = 256;

int64_t align_up(int64_t v) { return (v + ALIGN - 1) / ALIGN * ALIGN; }

// ---- the tensors the forward reads ---------------------------------------------------------------------------------------------
struct Spec { const char* name; int dtype; int ndim; int64_t shape[4]; };
#define W3(n, co, ci) {n ".weight", FLDR_MODEL_F32, 4, {co, ci, 3, 3}}, {n ".bias", FLDR_MODEL_F32, 1, {co}}
#define W4(n, co, ci) {n ".weight", FLDR_MODEL_F32, 4, {co, ci, 4, 4}}, {n ".bias", FLDR_MODEL_F32, 1, {co}}
const Spec SPECS[] = {
    {"EV8", FLDR_MODEL_F64, 2, {16, 64}}, {"Mean8", FLDR_MODEL_F64, 1, {64}}, {"meanVec8", FLDR_MODEL_F64, 1, {16}},
    W3("rec_ctx_ds.0", 96, 96), W3("rec_ctx_ds.2", 96, 96),
    {"vfinet.T_param", FLDR_MODEL_F64, 1, {1}}, {"vfinet.z_alpha", FLDR_MODEL_F64, 1, {2}},
    W3("vfinet.conv_flow_bottom.0", 96, 96), W3("vfinet.conv_flow_bottom.2", 96, 96), W3("vfinet.conv_flow_bottom.4", 96, 96),
    W3("vfinet.conv_flow_bottom.6", 48, 96), W3("vfinet.conv_flow_bottom.8", 6, 48),
    W3("vfinet.conv_flow1", 48, 96),
    W3("vfinet.conv_flow2.0", 96, 100), W3("vfinet.conv_flow2.2", 96, 96), W3("vfinet.conv_flow2.4", 48, 96),
    W3("vfinet.conv_flow2.6", 48, 48), W3("vfinet.conv_flow2.8", 4, 48),
    W4("vfinet.refine_unet.enc1", 16, 26), W4("vfinet.refine_unet.enc2", 32, 16), W4("vfinet.refine_unet.enc3", 64, 32),
    W3("vfinet.refine_unet.dec0", 64, 64), W3("vfinet.refine_unet.dec1", 32, 96), W3("vfinet.refine_unet.dec2", 16, 48),
    W3("vfinet.refine_unet.dec3", 6, 16),
};
#undef W3
#undef W4
constexpr int N_SPECS = sizeof(SPECS) / sizeof(SPECS[0]);
enum { T_EV, T_MEAN, T_MEANVEC, T_REC0W, T_REC0B, T_REC2W, T_REC2B, T_TPARAM, T_ZALPHA, T_BOT0W };   // the rest by name
const int T_BOTW[5] = {9, 11, 13, 15, 17};
const int T_FLOW1W = 19;
const int T_FLOW2W[5] = {21, 23, 25, 27, 29};
const int T_ENC1W = 31, T_ENC2W = 33, T_ENC3W = 35, T_DEC0W = 37, T_DEC1W = 39, T_DEC2W = 41, T_DEC3W = 43;

// the state dict also carries every module under its base_modules.* alias (fLDRnet.py:55-57)
std::string alias_of(const std::string& n) {
    if (n.rfind("rec_ctx_ds.", 0) == 0) return "base_modules.0." + n.substr(11);
    if (n.rfind("vfinet.", 0) == 0) return "base_modules.1." + n.substr(7);
    return std::string();
}

int64_t numel(const Spec& s) { int64_t n = 1; for (int i = 0; i < s.ndim; ++i) n *= s.shape[i]; return n; }

// host-only validation: every tensor the forward reads, present with its shape and dtype -> index per spec
int match_tensors(const fldr_model_tensor* t, int n, const fldr_model_tensor** found) {
    if (!t || n <= 0) return FLDR_MODEL_E_ARG;
    for (int s = 0; s < N_SPECS; ++s) {
        const std::string nm = SPECS[s].name, al = alias_of(nm);
        found[s] = nullptr;
        for (int i = 0; i < n && !found[s]; ++i)
            if (t[i].name && (nm == t[i].name || (!al.empty() && al == t[i].name))) found[s] = &t[i];
        if (!found[s]) return FLDR_MODEL_E_MISSING;
        const fldr_model_tensor& x = *found[s];
        if (!x.data) return FLDR_MODEL_E_ARG;
        if (x.dtype != SPECS[s].dtype) return FLDR_MODEL_E_DTYPE;
        if (x.ndim != SPECS[s].ndim) return FLDR_MODEL_E_TENSOR_SHAPE;
        for (int d = 0; d < x.ndim; ++d)
            if (x.shape[d] != SPECS[s].shape[d]) return FLDR_MODEL_E_TENSOR_SHAPE;
    }
    return 0;
}

// ---- .npz reader: an uncompressed zip of .npy files (np.savez) --------------------------------------------------------------------
uint16_t rd16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }
uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
uint64_t rd64(const uint8_t* p) { return (uint64_t)rd32(p) | ((uint64_t)rd32(p + 4) << 32); }

struct NpyEntry { std::string name; std::vector<int64_t> shape; int dtype; const uint8_t* data; };

// one .npy member: little-endian '<f4' / '<f8', C order
int parse_npy(const uint8_t* p, uint64_t size, NpyEntry& e) {
    if (size < 10) return FLDR_MODEL_E_TRUNCATED;
    if (memcmp(p, "\x93NUMPY", 6) != 0) return FLDR_MODEL_E_FORMAT;
    const int major = p[6];
    uint64_t hlen, hoff;
    if (major == 1) { hlen = rd16(p + 8); hoff = 10; }
    else if (major == 2 || major == 3) { if (size < 12) return FLDR_MODEL_E_TRUNCATED; hlen = rd32(p + 8); hoff = 12; }
    else return FLDR_MODEL_E_FORMAT;
    if (hoff + hlen > size) return FLDR_MODEL_E_TRUNCATED;
    const std::string h((const char*)p + hoff, (size_t)hlen);
    const size_t d = h.find("'descr'"), f = h.find("'fortran_order'"), s = h.find("'shape'");
    if (d == std::string::npos || f == std::string::npos || s == std::string::npos) return FLDR_MODEL_E_FORMAT;
    const size_t q0 = h.find('\'', h.find(':', d) + 1);
    const size_t q1 = q0 == std::string::npos ? q0 : h.find('\'', q0 + 1);
    if (q1 == std::string::npos) return FLDR_MODEL_E_FORMAT;
    const std::string descr = h.substr(q0 + 1, q1 - q0 - 1);
    if (descr == "<f4") e.dtype = FLDR_MODEL_F32;
    else if (descr == "<f8") e.dtype = FLDR_MODEL_F64;
    else e.dtype = -1;                                                   // reported as a dtype error if the forward reads it
    const size_t fv = h.find_first_not_of(" :", f + 15);
    if (fv == std::string::npos) return FLDR_MODEL_E_FORMAT;
    if (h.compare(fv, 4, "True") == 0) e.dtype = -1;
    const size_t b0 = h.find('(', s), b1 = b0 == std::string::npos ? b0 : h.find(')', b0);
    if (b1 == std::string::npos) return FLDR_MODEL_E_FORMAT;
    e.shape.clear();
    const char* c = h.c_str() + b0 + 1;
    const char* end = h.c_str() + b1;
    while (c < end) {
        while (c < end && (*c == ' ' || *c == ',')) ++c;
        if (c >= end) break;
        char* nx;
        const long long v = strtoll(c, &nx, 10);
        if (nx == c || v < 0) return FLDR_MODEL_E_FORMAT;
        e.shape.push_back(v);
        c = nx;
    }
    int64_t n = 1;
    for (int64_t v : e.shape) n *= v;
    const uint64_t need = (uint64_t)n * (e.dtype == FLDR_MODEL_F64 ? 8 : 4);
    if (e.dtype >= 0 && hoff + hlen + need > size) return FLDR_MODEL_E_TRUNCATED;
    e.data = p + hoff + hlen;
    return 0;
}

int parse_npz(const std::vector<uint8_t>& f, std::vector<NpyEntry>& out) {
    const uint64_t n = f.size();
    const uint8_t* b = f.data();
    const bool starts_zip = n >= 4 && rd32(b) == 0x04034b50u;
    // end of central directory: the last 22+ bytes (comment up to 64 KB)
    int64_t eocd = -1;
    for (int64_t i = (int64_t)n - 22; i >= 0 && i >= (int64_t)n - 22 - 65535; --i)
        if (rd32(b + i) == 0x06054b50u) { eocd = i; break; }
    if (eocd < 0) return starts_zip ? FLDR_MODEL_E_TRUNCATED : FLDR_MODEL_E_FORMAT;
    uint64_t count = rd16(b + eocd + 10), cd_size = rd32(b + eocd + 12), cd_off = rd32(b + eocd + 16);
    if (cd_off == 0xffffffffu || count == 0xffffu) {                      // zip64 end record through its locator
        if (eocd < 20 || rd32(b + eocd - 20) != 0x07064b50u) return FLDR_MODEL_E_FORMAT;
        const uint64_t z = rd64(b + eocd - 20 + 8);
        if (z + 56 > n || rd32(b + z) != 0x06064b50u) return FLDR_MODEL_E_TRUNCATED;
        count = rd64(b + z + 32); cd_size = rd64(b + z + 40); cd_off = rd64(b + z + 48);
    }
    if (cd_off + cd_size > n) return FLDR_MODEL_E_TRUNCATED;
    uint64_t p = cd_off;
    for (uint64_t k = 0; k < count; ++k) {
        if (p + 46 > n) return FLDR_MODEL_E_TRUNCATED;
        if (rd32(b + p) != 0x02014b50u) return FLDR_MODEL_E_FORMAT;
        const int method = rd16(b + p + 10);
        uint64_t csize = rd32(b + p + 20), usize = rd32(b + p + 24), loff = rd32(b + p + 42);
        const int nlen = rd16(b + p + 28), xlen = rd16(b + p + 30), clen = rd16(b + p + 32);
        if (p + 46 + nlen + xlen + clen > n) return FLDR_MODEL_E_TRUNCATED;
        std::string name((const char*)b + p + 46, nlen);
        // zip64 extra field: the 0xffffffff fields, in the order usize, csize, local offset
        for (uint64_t x = p + 46 + nlen; x + 4 <= p + 46 + nlen + xlen;) {
            const int id = rd16(b + x), len = rd16(b + x + 2);
            if (id == 1) {
                uint64_t q = x + 4;
                if (usize == 0xffffffffu && q + 8 <= x + 4 + len) { usize = rd64(b + q); q += 8; }
                if (csize == 0xffffffffu && q + 8 <= x + 4 + len) { csize = rd64(b + q); q += 8; }
                if (loff == 0xffffffffu && q + 8 <= x + 4 + len) { loff = rd64(b + q); q += 8; }
            }
            x += 4 + len;
        }
        p += 46 + nlen + xlen + clen;
        if (method != 0) return FLDR_MODEL_E_COMPRESSED;
        if (csize != usize) return FLDR_MODEL_E_FORMAT;
        if (loff + 30 > n) return FLDR_MODEL_E_TRUNCATED;
        if (rd32(b + loff) != 0x04034b50u) return FLDR_MODEL_E_FORMAT;
        const uint64_t data = loff + 30 + rd16(b + loff + 26) + rd16(b + loff + 28);
        if (data + usize > n) return FLDR_MODEL_E_TRUNCATED;
        if (name.size() <= 4 || name.compare(name.size() - 4, 4, ".npy") != 0) continue;     // not an array (np.load keeps such members as bytes)
        name.resize(name.size() - 4);
        NpyEntry e;
        e.name = name;
        const int rc = parse_npy(b + data, usize, e);
        if (rc) return rc;
        out.push_back(e);
    }
    return 0;
}

// ---- workspace layout ---------------------------------------------------------------------------------------------------------
struct Layout {
    int S, n_levels, H, W, Hp, Wp;
    int lh[FLDR_MODEL_MAX_LEVELS], lw[FLDR_MODEL_MAX_LEVELS];    // pyramid level size
    int fh[FLDR_MODEL_MAX_LEVELS], fw[FLDR_MODEL_MAX_LEVELS];    // feature / flow size (level / 8)
    int64_t pyr[FLDR_MODEL_MAX_LEVELS], pca32[FLDR_MODEL_MAX_LEVELS], pcasp[FLDR_MODEL_MAX_LEVELS], raw[FLDR_MODEL_MAX_LEVELS], minmax;
    int64_t ys[FLDR_MODEL_MAX_LEVELS], feat32[FLDR_MODEL_MAX_LEVELS], featsp[FLDR_MODEL_MAX_LEVELS];
    int64_t chain[FLDR_MODEL_MAX_LEVELS][4], flow[FLDR_MODEL_MAX_LEVELS];
    int64_t up[FLDR_MODEL_MAX_LEVELS], upsp[FLDR_MODEL_MAX_LEVELS], bw[FLDR_MODEL_MAX_LEVELS], wpair[FLDR_MODEL_MAX_LEVELS], pair[FLDR_MODEL_MAX_LEVELS];
    int64_t z0, z1, ft0, ft1, fb0, fb1, it0, it1, prepws, bwimg, warp0, warp1, enc1p, enc2p, enc3p[2], dec0p, dec1p, f64, u8;
    int64_t total;
};

int64_t spk(int C, int H, int W) { return fldr_spk_bytes(C, H, W); }

int plan(int S, int H, int W, int n_t, Layout& L) {
    if (H < 2 || W < 2 || n_t < 1) return FLDR_MODEL_E_ARG;
    const int div = (1 << S) * 8;
    L.S = S; L.n_levels = S + 1; L.H = H; L.W = W;
    L.Hp = (H + div - 1) / div * div; L.Wp = (W + div - 1) / div * div;
    if (L.Hp - H >= H || L.Wp - W >= W) return FLDR_MODEL_E_SHAPE;       // reflect padding needs pad < size (main.py:848)
    int64_t o = 0;
    auto take = [&](int64_t bytes) { const int64_t r = o; o += align_up(bytes > 0 ? bytes : 1); return r; };
    const int64_t HW = (int64_t)L.Hp * L.Wp;
    for (int i = 0; i < L.n_levels; ++i) {
        L.lh[i] = L.Hp >> i; L.lw[i] = L.Wp >> i; L.fh[i] = L.lh[i] / 8; L.fw[i] = L.lw[i] / 8;
        const int64_t f = (int64_t)L.fh[i] * L.fw[i];
        L.pyr[i] = take(6ll * L.lh[i] * L.lw[i] * 4);
        L.pca32[i] = take(NCH * f * 4);
        L.pcasp[i] = take(spk(NCH, L.fh[i], L.fw[i]));
        L.raw[i] = take(6 * f * K_PCA * 8);
        L.ys[i] = take(spk(NCH, L.fh[i], L.fw[i]));
        L.feat32[i] = take(NCH * f * 4);
        L.featsp[i] = take(spk(NCH, L.fh[i], L.fw[i]));
        const int cc[4] = {NCH, NCH, i == S ? NCH : HALF, HALF};          // bottom: 96 96 96 48; conv_flow2: 96 96 48 48
        for (int k = 0; k < 4; ++k) L.chain[i][k] = take(spk(cc[k], L.fh[i], L.fw[i]));
        L.flow[i] = take(4 * f * 4);
        L.up[i] = take(4 * f * 4);
        L.upsp[i] = take(spk(4, L.fh[i], L.fw[i]));
        L.bw[i] = take(2 * fldr_softsplat_tile_ws_floats(1, L.fh[i], L.fw[i]) * 4);
        L.wpair[i] = take(2 * spk(HALF, L.fh[i], L.fw[i]));
        L.pair[i] = take(2 * spk(HALF, L.fh[i], L.fw[i]));
    }
    L.minmax = take(32ll * L.n_levels * 8);
    L.z0 = take(HW * 4); L.z1 = take(HW * 4);
    L.ft0 = take(2 * HW * 4); L.ft1 = take(2 * HW * 4); L.fb0 = take(2 * HW * 4); L.fb1 = take(2 * HW * 4);
    L.it0 = take(3 * HW * 4); L.it1 = take(3 * HW * 4);
    L.prepws = take((int64_t)L.fh[0] * L.fw[0] * 4 * 4);
    L.bwimg = take(2 * fldr_softsplat_tile_ws_floats(1, L.Hp, L.Wp) * 4);
    L.warp0 = take(3 * HW * 4); L.warp1 = take(3 * HW * 4);
    L.enc1p = take(spk(16, L.Hp / 2, L.Wp / 2));
    L.enc2p = take(spk(32, L.Hp / 4, L.Wp / 4));
    L.enc3p[0] = take(spk(32, L.Hp / 8, L.Wp / 8)); L.enc3p[1] = take(spk(32, L.Hp / 8, L.Wp / 8));
    L.dec0p = take(spk(64, L.Hp / 8, L.Wp / 8));
    L.dec1p = take(spk(32, L.Hp / 4, L.Wp / 4));
    L.f64 = (W & 1) ? take(3 * HW * 8) : -1;                             // odd widths: the 8-bit frame from the fp64 one (fldr_frame_metrics)
    L.u8 = take(3ll * H * W);                                             // planar 8-bit frame in front of the interleaving kernel
    L.total = o;
    return 0;
}

struct Conv { const float* wpack; const float* bias; int cout, cin; };

}  // namespace

struct fldr_model {
    int device, S;
    void* mem;
    const double* pca_table;
    Conv rec0, rec2, bottom[5], flow1, flow2[5], dec0, dec1, enc1, enc2, enc3[2];
    const float* w2pack; const float* bias2; const float* w3m; const float* bias3;
    double T;
    float za0, za1;
    const volatile int* status;
};

// ---- public functions ----------------------------------------------------------------------------------------------------------
extern "C" FLDR_MODEL_API int fldr_model_version(void) { return FLDR_MODEL_VERSION; }

extern "C" FLDR_MODEL_API const char* fldr_model_error_string(int code) {
    switch (code) {
    case 0: return "success";
    case FLDR_MODEL_E_ARG: return "fldr_model: bad argument";
    case FLDR_MODEL_E_SHAPE: return "fldr_model: frame size not supported";
    case FLDR_MODEL_E_STATUS: return "fldr_model: a device fault flag is set (or the status block could not be bound)";
    case FLDR_MODEL_E_WORKSPACE: return "fldr_model: workspace too small";
    case FLDR_MODEL_E_BATCH: return "fldr_model: batch must be 1";
    case FLDR_MODEL_E_IO: return "fldr_model: cannot read the file";
    case FLDR_MODEL_E_FORMAT: return "fldr_model: not an uncompressed zip of .npy files";
    case FLDR_MODEL_E_COMPRESSED: return "fldr_model: compressed .npz entry";
    case FLDR_MODEL_E_TRUNCATED: return "fldr_model: truncated file";
    case FLDR_MODEL_E_MISSING: return "fldr_model: missing tensor";
    case FLDR_MODEL_E_TENSOR_SHAPE: return "fldr_model: tensor of the wrong shape";
    case FLDR_MODEL_E_DTYPE: return "fldr_model: tensor of the wrong dtype";
    case FLDR_MODEL_E_DEVICE: return "fldr_model: no such device or out of device memory";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "fldr_model: unknown error";
    }
}

extern "C" FLDR_MODEL_API int fldr_model_sizeof(int which) {
    switch (which) {
    case 0: return (int)sizeof(fldr_model_tensor);
    case 1: return (int)sizeof(fldr_model_config);
    case 2: return (int)sizeof(fldr_model_io);
    default: return FLDR_MODEL_E_ARG;
    }
}

namespace {

struct DeviceGuard {                                      // make `dev` current, restore the caller's device on exit
    int prev = -1;
    int rc = 0;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev && hipSetDevice(dev) != hipSuccess) rc = FLDR_MODEL_E_DEVICE;
    }
    ~DeviceGuard() { if (prev >= 0) { int cur = -1; if (hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev); } }
};

int create_on_device(const fldr_model_tensor** t, int device, int S, fldr_model* m) {
    hipStream_t s = nullptr;
    // device layout: every tensor as uploaded, then the prepacks
    std::vector<int64_t> off(N_SPECS);
    int64_t o = 0;
    for (int i = 0; i < N_SPECS; ++i) { off[i] = o; o += align_up(numel(SPECS[i]) * (SPECS[i].dtype == FLDR_MODEL_F64 ? 8 : 4)); }
    struct Pack { int w; int64_t n; int kind; int part; int64_t off; };   // kind 0: spk 3x3, 1: s2 4x4, 2: dec23, 3: dec3 spk, 4: pca table
    std::vector<Pack> packs;
    auto add = [&](int w, int64_t n, int kind, int part) { packs.push_back({w, n, kind, part, o}); o += align_up(n * (kind == 4 ? 8 : 4)); };
    const int spk3[] = {T_REC0W, T_REC2W, T_BOTW[0], T_BOTW[1], T_BOTW[2], T_BOTW[3], T_BOTW[4], T_FLOW1W,
                        T_FLOW2W[0], T_FLOW2W[1], T_FLOW2W[2], T_FLOW2W[3], T_FLOW2W[4], T_DEC0W, T_DEC1W};
    for (int w : spk3) add(w, fldr_conv_spk_prepack_size((int)SPECS[w].shape[0], (int)SPECS[w].shape[1]), 0, 0);
    add(T_ENC1W, fldr_conv_s2_prepack_size(16, 26), 1, 0);
    add(T_ENC2W, fldr_conv_s2_prepack_size(32, 16), 1, 0);
    add(T_ENC3W, fldr_conv_s2_prepack_size(32, 32), 1, 0);              // enc3 as two halves of 32 output channels (fLDRnet.py _enc3_halves)
    add(T_ENC3W, fldr_conv_s2_prepack_size(32, 32), 1, 1);
    add(T_DEC2W, fldr_dec23_prepack_size(), 2, 0);
    add(T_DEC3W, fldr_dec3_prepack_spk_size(), 3, 0);
    add(T_EV, fldr_pca_table_size(K_PCA), 4, 0);
    for (const Pack& p : packs) if (p.n <= 0) return FLDR_MODEL_E_ARG;
    if (hipMalloc(&m->mem, (size_t)o) != hipSuccess) { m->mem = nullptr; (void)hipGetLastError(); return FLDR_MODEL_E_DEVICE; }
    char* base = (char*)m->mem;
    for (int i = 0; i < N_SPECS; ++i) {
        const hipError_t e = hipMemcpy(base + off[i], t[i]->data, (size_t)numel(SPECS[i]) * (SPECS[i].dtype == FLDR_MODEL_F64 ? 8 : 4), hipMemcpyHostToDevice);
        if (e != hipSuccess) return (int)e;
    }
    auto F = [&](int i) { return (const float*)(base + off[i]); };
    auto D = [&](int i) { return (const double*)(base + off[i]); };
    int rc = 0;
    std::vector<const float*> packed(packs.size());
    for (size_t k = 0; k < packs.size() && !rc; ++k) {
        const Pack& p = packs[k];
        float* dst = (float*)(base + p.off);
        packed[k] = dst;
        const int co = (int)SPECS[p.w].shape[0], ci = (int)SPECS[p.w].shape[1];
        switch (p.kind) {
        case 0: rc = fldr_conv_spk_prepack(F(p.w), dst, co, ci, s); break;
        case 1: rc = p.w == T_ENC3W ? fldr_conv_s2_prepack(F(p.w) + (int64_t)p.part * 32 * 32 * 16, dst, 32, 32, s)
                                    : fldr_conv_s2_prepack(F(p.w), dst, co, ci, s); break;
        case 2: rc = fldr_dec23_prepack(F(p.w), dst, s); break;
        case 3: rc = fldr_dec3_prepack_spk(F(p.w), dst, s); break;
        case 4: rc = fldr_pca_prepack(D(T_EV), D(T_MEAN), D(T_MEANVEC), (double*)dst, K_PCA, s); break;
        }
    }
    if (rc) return rc;
    const hipError_t se = hipStreamSynchronize(s);
    if (se != hipSuccess) return (int)se;
    auto conv = [&](int w, size_t k) { return Conv{packed[k], F(w + 1), (int)SPECS[w].shape[0], (int)SPECS[w].shape[1]}; };
    m->rec0 = conv(T_REC0W, 0); m->rec2 = conv(T_REC2W, 1);
    for (int i = 0; i < 5; ++i) m->bottom[i] = conv(T_BOTW[i], 2 + i);
    m->flow1 = conv(T_FLOW1W, 7);
    for (int i = 0; i < 5; ++i) m->flow2[i] = conv(T_FLOW2W[i], 8 + i);
    m->dec0 = conv(T_DEC0W, 13); m->dec1 = conv(T_DEC1W, 14);
    m->enc1 = conv(T_ENC1W, 15); m->enc2 = conv(T_ENC2W, 16);
    m->enc3[0] = Conv{packed[17], F(T_ENC3W + 1), 32, 32};
    m->enc3[1] = Conv{packed[18], F(T_ENC3W + 1) + 32, 32, 32};
    m->w2pack = packed[19]; m->bias2 = F(T_DEC2W + 1);
    m->w3m = packed[20]; m->bias3 = F(T_DEC3W + 1);
    m->pca_table = (const double*)packed[21];
    // T_param / z_alpha on the host (DCTVFInet._host_scalars); z_alpha reaches the kernel as fp32 like the ctypes float of fldr_hip.level0_prep
    m->T = ((const double*)t[T_TPARAM]->data)[0];
    m->za0 = (float)((const double*)t[T_ZALPHA]->data)[0];
    m->za1 = (float)((const double*)t[T_ZALPHA]->data)[1];
    // bind the status block now: no forward then runs a kernel before it is bound, and none allocates or synchronises
    const volatile int* words = nullptr;
    rc = fldr_status_word(&words);
    if (rc || !words) return rc ? rc : FLDR_MODEL_E_STATUS;
    m->status = words;
    m->device = device;
    m->S = S;
    return 0;
}

}  // namespace

extern "C" FLDR_MODEL_API int fldr_model_create(const fldr_model_tensor* tensors, int n, const fldr_model_config* cfg, fldr_model** out) {
    if (!out) return FLDR_MODEL_E_ARG;
    *out = nullptr;
    if (!cfg) return FLDR_MODEL_E_ARG;
    const int S = cfg->test_scales == 0 ? 5 : cfg->test_scales;
    if (S < 3 || S > 7 || cfg->device < 0) return FLDR_MODEL_E_ARG;
    for (int i = 0; i < 6; ++i) if (cfg->reserved[i]) return FLDR_MODEL_E_ARG;
    const fldr_model_tensor* found[N_SPECS];
    const int v = match_tensors(tensors, n, found);                       // host only: nothing has touched the device yet
    if (v) return v;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device >= ndev) { (void)hipGetLastError(); return FLDR_MODEL_E_DEVICE; }
    fldr_model* m = new fldr_model();
    m->mem = nullptr;
    int rc;
    {
        DeviceGuard g(cfg->device);
        rc = g.rc ? g.rc : create_on_device(found, cfg->device, S, m);
        if (rc && m->mem) (void)hipFree(m->mem);
    }
    if (rc) { delete m; return rc; }
    *out = m;
    return 0;
}

extern "C" FLDR_MODEL_API int fldr_model_create_npz(const char* path, const fldr_model_config* cfg, fldr_model** out) {
    if (!out) return FLDR_MODEL_E_ARG;
    *out = nullptr;
    if (!path || !cfg) return FLDR_MODEL_E_ARG;
    FILE* fp = fopen(path, "rb");
    if (!fp) return FLDR_MODEL_E_IO;
    std::vector<uint8_t> buf;
    if (fseek(fp, 0, SEEK_END) == 0) {
        const long sz = ftell(fp);
        if (sz > 0 && fseek(fp, 0, SEEK_SET) == 0) {
            buf.resize((size_t)sz);
            if (fread(buf.data(), 1, buf.size(), fp) != buf.size()) buf.clear();
        }
    }
    fclose(fp);
    if (buf.empty()) return FLDR_MODEL_E_IO;
    std::vector<NpyEntry> entries;
    const int rc = parse_npz(buf, entries);
    if (rc) return rc;
    std::vector<fldr_model_tensor> ts(entries.size());
    for (size_t i = 0; i < entries.size(); ++i) {
        fldr_model_tensor& t = ts[i];
        memset(&t, 0, sizeof(t));
        t.name = entries[i].name.c_str();
        t.data = entries[i].data;
        t.dtype = entries[i].dtype;
        t.ndim = (int)entries[i].shape.size();
        if (t.ndim > 4) t.ndim = 5;                                          // never a match: reported as a shape error if read
        for (int d = 0; d < 4 && d < (int)entries[i].shape.size(); ++d) t.shape[d] = entries[i].shape[d];
    }
    if (ts.empty()) return FLDR_MODEL_E_MISSING;
    // the .npy data inside the zip need not be aligned for its dtype: hipMemcpy takes any host address
    return fldr_model_create(ts.data(), (int)ts.size(), cfg, out);
}

extern "C" FLDR_MODEL_API void fldr_model_destroy(fldr_model* m) {
    if (!m) return;
    {
        DeviceGuard g(m->device);
        if (m->mem) (void)hipFree(m->mem);
    }
    delete m;
}

extern "C" FLDR_MODEL_API int64_t fldr_model_workspace_bytes(const fldr_model* m, int H, int W, int n_t) {
    if (!m) return FLDR_MODEL_E_ARG;
    Layout L;
    const int rc = plan(m->S, H, W, n_t, L);
    return rc ? rc : L.total;
}

namespace {

#define CK(x) do { const int rc_ = (x); if (rc_) return rc_; } while (0)

constexpr int U10_MAX = 1023;          // white level of the 10-bit forms

fldr_spk_conv_desc spk_desc(const Conv& c, int N, int H, int W, int relu) {
    fldr_spk_conv_desc d;
    memset(&d, 0, sizeof(d));
    d.wpack = c.wpack; d.bias = c.bias;
    d.N = N; d.cin = c.cin; d.cout = c.cout; d.cout_store = c.cout;
    d.H = H; d.W = W; d.relu = relu; d.precision = 0;
    return d;
}
void add_src(fldr_spk_conv_desc& d, const void* p, int64_t bstride, int c, int up2) {
    d.src[d.n_src] = p; d.src_bstride[d.n_src] = bstride; d.src_c[d.n_src] = c; d.src_up2[d.n_src] = up2; ++d.n_src;
}

// the 3x3 chains of DCTVFInet._chain: every convolution but the last with ReLU and a packed output, the last fp32
int chain(const Conv* convs, const void* const* first_src, const int* first_c, int n_first, char* ws, const Layout& L, int l,
          float* out, int cout_store, const float* residual, hipStream_t s) {
    const int h = L.fh[l], w = L.fw[l];
    const void* prev = nullptr;
    for (int k = 0; k < 5; ++k) {
        const bool last = k == 4;
        fldr_spk_conv_desc d = spk_desc(convs[k], 1, h, w, last ? 0 : 1);
        if (k == 0) for (int i = 0; i < n_first; ++i) add_src(d, first_src[i], 0, first_c[i], 0);
        else add_src(d, prev, 0, convs[k].cin, 0);
        if (last) { d.out_f32 = out; d.cout_store = cout_store; d.residual = residual; }
        else { d.out_spk = ws + L.chain[l][k]; prev = d.out_spk; }
        CK(fldr_conv2d_spk(&d, s));
    }
    return 0;
}

int enqueue(const fldr_model* m, const fldr_model_io* io, char* ws, const Layout& L, hipStream_t s) {
    const int n = L.n_levels, Hp = L.Hp, Wp = L.Wp;
    const int64_t HW = (int64_t)Hp * Wp;
    // ---- the frame pyramid (normInput): main.py:840-856 ----
    float* lv[FLDR_MODEL_MAX_LEVELS];
    for (int i = 0; i < n; ++i) lv[i] = io->pyramid[i] ? (float*)io->pyramid[i] : (float*)(ws + L.pyr[i]);     // 8-bit inputs: ingested there
    if (io->input == FLDR_MODEL_IN_U8_PLANAR) {                         // fldr_hip.ingest_pyramid
        if (n <= 7) CK(fldr_ingest_pyramid_u8(io->frames_u8, lv, n, 1, L.H, L.W, Hp, Wp, s));
        else {
            CK(fldr_ingest_u8(io->frames_u8, lv[0], 1, L.H, L.W, Hp, Wp, s));
            for (int i = 1; i < n; ++i) CK(fldr_pyramid_bicubic(lv[0], lv[i], 6, Hp, Wp, 1 << i, s));
        }
    } else if (io->input == FLDR_MODEL_IN_U10_PLANAR) {                 // fldr_hip.ingest_pyramid_u16
        const uint16_t* u16 = (const uint16_t*)io->frames_u8;
        if (n <= 7) CK(fldr_ingest_pyramid_u16(u16, lv, n, U10_MAX, 1, L.H, L.W, Hp, Wp, s));
        else {
            CK(fldr_ingest_u16(u16, lv[0], U10_MAX, 1, L.H, L.W, Hp, Wp, s));
            for (int i = 1; i < n; ++i) CK(fldr_pyramid_bicubic(lv[0], lv[i], 6, Hp, Wp, 1 << i, s));
        }
    } else if (io->input == FLDR_MODEL_IN_U8_INTERLEAVED) {
        const int nk = n < MI_MAX_LEVELS ? n : MI_MAX_LEVELS;
        CK(ingest_interleaved_pyramid(io->frame, io->frame_pitch, io->in_order == FLDR_MODEL_RGB, lv, nk, L.H, L.W, Hp, Wp, s));
        for (int i = nk; i < n; ++i) CK(fldr_pyramid_bicubic(lv[0], lv[i], 6, Hp, Wp, 1 << i, s));   // depth 7: the 128x level from level 0
    }
    // ---- PCA features of every level in two launches (fLDRnet.py:133-146; to_pca_diff_f32_pyramid) ----
    fldr_pca_level pl[FLDR_MODEL_MAX_LEVELS];
    memset(pl, 0, sizeof(pl));
    for (int i = 0; i < n; ++i) {
        pl[i].planes = lv[i]; pl[i].out_f32 = (float*)(ws + L.pca32[i]); pl[i].out_spk = ws + L.pcasp[i];
        pl[i].P = 6; pl[i].H = L.lh[i]; pl[i].W = L.lw[i]; pl[i].raw_ws = (double*)(ws + L.raw[i]);
    }
    CK(fldr_pca_project_pyramid(pl, n, m->pca_table, K_PCA, (double*)(ws + L.minmax), s));
    // ---- rec_ctx_ds(x) + x of all levels in two launches (fLDRnet.py:148-162) ----
    fldr_spk_conv_desc dl[FLDR_MODEL_MAX_LEVELS];
    for (int i = 0; i < n; ++i) {
        dl[i] = spk_desc(m->rec0, 1, L.fh[i], L.fw[i], 1);
        add_src(dl[i], ws + L.pcasp[i], 0, NCH, 0);
        dl[i].out_spk = ws + L.ys[i];
    }
    CK(fldr_conv2d_spk_levels(dl, n, s));
    for (int i = 0; i < n; ++i) {
        dl[i] = spk_desc(m->rec2, 1, L.fh[i], L.fw[i], 1);
        add_src(dl[i], ws + L.ys[i], 0, NCH, 0);
        dl[i].residual = (const float*)(ws + L.pca32[i]);
        dl[i].out_f32 = (float*)(ws + L.feat32[i]);
        dl[i].out_spk = ws + L.featsp[i];
    }
    CK(fldr_conv2d_spk_levels(dl, n, s));
    // ---- flow estimation, coarsest level first (fLDRnet.py:210-218, DCTVFInet.estimate_flow) ----
    {
        const void* src[1] = {ws + L.featsp[L.S]};
        const int c[1] = {NCH};
        CK(chain(m->bottom, src, c, 1, ws, L, L.S, (float*)(ws + L.flow[L.S]), 4, nullptr, s));
    }
    for (int l = L.S - 1; l >= 0; --l) {
        const int h = L.fh[l], w = L.fw[l], ph = L.fh[l + 1], pw = L.fw[l + 1];
        const int64_t f = (int64_t)h * w;
        const float mul = (float)((double)w / pw);
        const float* prev = (const float*)(ws + L.flow[l + 1]);
        float* up = (float*)(ws + L.up[l]);
        void* upsp = ws + L.upsp[l];
        float* bw = nullptr;
        if (f > 2304) {
            bw = (float*)(ws + L.bw[l]);
            if (w >= 4 * pw) {
                CK(fldr_resize_bilinear_spk(prev, up, upsp, 1, 4, ph, pw, h, w, mul, s));
                CK(fldr_splat_bounds_upsampled_pair(prev, 0, nullptr, 2, mul, bw, 1, ph, pw, h, w, s));
            } else {
                CK(fldr_resize_bilinear_spk_bounds(prev, up, upsp, bw, 1, ph, pw, h, w, mul, s));
            }
        } else {
            CK(fldr_resize_bilinear_spk(prev, up, upsp, 1, 4, ph, pw, h, w, mul, s));
        }
        // both feature splats in one launch, packed into one batch of two (sample 0: feat1 along up[:, :2], 1: feat0 along up[:, 2:])
        const float* feat = (const float*)(ws + L.feat32[l]);
        const int64_t s48 = spk(HALF, h, w);
        char* wpair = ws + L.wpair[l];
        fldr_splat_acc_desc a;
        memset(&a, 0, sizeof(a));
        a.img[0] = feat + HALF * f; a.img[1] = feat;
        a.img_cstride[0] = a.img_cstride[1] = f;
        a.flow[0] = up; a.flow[1] = up + 2 * f;
        a.ws[0] = a.ws[1] = bw;
        a.out_spk[0] = wpair; a.out_spk[1] = wpair + s48;
        a.nprob = 2; a.N = 1; a.C = HALF; a.H = h; a.W = w; a.mode = 3; a.flags = bw ? 2 : 0;
        CK(fldr_softsplat_acc64(&a, s));
        // conv_flow1 of (feat0, w1) and (feat1, w0) as one batch of two
        char* pair = ws + L.pair[l];
        fldr_spk_conv_desc d = spk_desc(m->flow1, 2, h, w, 0);
        add_src(d, ws + L.featsp[l], s48, HALF, 0);
        add_src(d, wpair, s48, HALF, 0);
        d.out_spk = pair;
        CK(fldr_conv2d_spk(&d, s));
        const void* src[3] = {pair, pair + s48, upsp};
        const int c[3] = {HALF, HALF, 4};
        CK(chain(m->flow2, src, c, 3, ws, L, l, (float*)(ws + L.flow[l]), 4, up, s));
    }
    // ---- level 0, once per output (DCTVFInet._synthesise); z0 / z1 do not depend on t: computed for the first output only ----
    const float* flow0 = (const float*)(ws + L.flow[0]);
    const float* I0 = lv[0];
    const float* I1 = lv[0] + HW;
    float* z0 = (float*)(ws + L.z0); float* z1 = (float*)(ws + L.z1);
    float* ft0 = (float*)(ws + L.ft0); float* ft1 = (float*)(ws + L.ft1);
    float* fb0 = (float*)(ws + L.fb0); float* fb1 = (float*)(ws + L.fb1);
    float* it0 = (float*)(ws + L.it0); float* it1 = (float*)(ws + L.it1);
    float* w0 = (float*)(ws + L.warp0); float* w1 = (float*)(ws + L.warp1);
    float* bwimg = (float*)(ws + L.bwimg);
    const float up0 = (float)((double)Hp / L.fh[0]);
    // The rounded output forms hold the frame's own L.H rows: every stage below produces only the rows those need (fldr_synth_row_plan) and
    // leaves the padded rows under them untouched.  FLDR_MODEL_OUT_F64 is the whole padded frame: no limit (all zeros = all rows).
    fldr_synth_rows rows;
    memset(&rows, 0, sizeof(rows));
    int src1 = 0;                                                        // rows of the frame-resolution planes enc1 may read
    if (io->output != FLDR_MODEL_OUT_F64 && L.H < Hp) {
        CK(fldr_synth_row_plan(Hp, L.H, &rows));
        src1 = rows.prep2 < rows.splat ? rows.prep2 : rows.splat;
    }
    for (int k = 0; k < io->n_t; ++k) {
        const float* t = io->t + k;
        fldr_prep_desc p;
        memset(&p, 0, sizeof(p));
        p.flow_lo = flow0; p.I0 = I0; p.I1 = I1; p.t = t;
        p.z0 = k == 0 ? z0 : nullptr; p.z1 = k == 0 ? z1 : nullptr;
        p.flow_t0 = ft0; p.flow_t1 = ft1; p.flowback_0 = fb0; p.flowback_1 = fb1; p.im0_tot = it0; p.im1_tot = it1;
        p.N = 1; p.h = L.fh[0]; p.w = L.fw[0]; p.H = Hp; p.W = Wp;
        p.mul = up0; p.z_alpha0 = m->za0; p.z_alpha1 = m->za1; p.withmask = 1;
        p.ws = (float*)(ws + L.prepws);
        p.i0_cstride = p.i1_cstride = 2 * HW;
        p.phase = 3;
        p.reserved = rows.prep2;
        CK(fldr_level0_prep(&p, s));
        CK(fldr_splat_bounds_upsampled_pair(flow0, 0, t, 1, up0, bwimg, 1, L.fh[0], L.fw[0], Hp, Wp, s));
        fldr_splat_acc_desc a;
        memset(&a, 0, sizeof(a));
        a.img[0] = I0; a.img[1] = I1; a.img_cstride[0] = a.img_cstride[1] = 2 * HW;
        a.flow[0] = ft0; a.flow[1] = ft1;
        a.metric[0] = z0; a.metric[1] = z1;
        a.ws[0] = a.ws[1] = bwimg;
        a.out_f32[0] = w0; a.out_f32[1] = w1;
        a.nprob = 2; a.N = 1; a.C = 3; a.H = Hp; a.W = Wp; a.mode = 3; a.flags = 2;
        a.reserved = rows.splat;
        CK(fldr_softsplat_acc64(&a, s));
        // PCARefineUNet up to dec1 (forward_until_dec1): enc1 on the 26 planes of fLDRnet.py:480, never concatenated
        fldr_conv_desc e;
        memset(&e, 0, sizeof(e));
        const float* srcs[10] = {I0, I1, w0, w1, ft0, ft1, fb0, fb1, it0, it1};
        const int cs[10] = {3, 3, 3, 3, 2, 2, 2, 2, 3, 3};
        for (int i = 0; i < 10; ++i) { e.src[i] = srcs[i]; e.src_c[i] = cs[i]; e.src_cstride[i] = i < 2 ? 2 * HW : HW; }
        e.n_src = 10; e.wpack = m->enc1.wpack; e.bias = m->enc1.bias; e.out_spk = ws + L.enc1p;
        e.N = 1; e.cin = 26; e.cout = 16; e.cout_store = 16; e.Hin = Hp; e.Win = Wp; e.Hout = Hp / 2; e.Wout = Wp / 2;
        e.ksize = 4; e.stride = 2; e.relu = 1; e.precision = 0;
        CK(fldr_conv2d_s2_split_rows(&e, rows.enc1, src1, s));
        fldr_conv_desc e2;
        memset(&e2, 0, sizeof(e2));
        e2.src[0] = (const float*)(ws + L.enc1p); e2.src_c[0] = 16; e2.n_src = 1;
        e2.wpack = m->enc2.wpack; e2.bias = m->enc2.bias; e2.out_spk = ws + L.enc2p;
        e2.N = 1; e2.cin = 16; e2.cout = 32; e2.cout_store = 32; e2.Hin = Hp / 2; e2.Win = Wp / 2; e2.Hout = Hp / 4; e2.Wout = Wp / 4;
        e2.ksize = 4; e2.stride = 2; e2.relu = 1;
        CK(fldr_conv2d_s2_spk_rows(&e2, rows.enc2, rows.enc1, s));
        fldr_conv_desc e3[2];
        for (int hf = 0; hf < 2; ++hf) {
            memset(&e3[hf], 0, sizeof(e3[hf]));
            e3[hf].src[0] = (const float*)(ws + L.enc2p); e3[hf].src_c[0] = 32; e3[hf].n_src = 1;
            e3[hf].wpack = m->enc3[hf].wpack; e3[hf].bias = m->enc3[hf].bias; e3[hf].out_spk = ws + L.enc3p[hf];
            e3[hf].N = 1; e3[hf].cin = 32; e3[hf].cout = 32; e3[hf].cout_store = 32;
            e3[hf].Hin = Hp / 4; e3[hf].Win = Wp / 4; e3[hf].Hout = Hp / 8; e3[hf].Wout = Wp / 8;
            e3[hf].ksize = 4; e3[hf].stride = 2; e3[hf].relu = 1;
        }
        CK(fldr_conv2d_s2_spk_pair_rows(&e3[0], &e3[1], rows.enc3, rows.enc2, s));
        fldr_spk_conv_desc d0 = spk_desc(m->dec0, 1, Hp / 8, Wp / 8, 1);
        add_src(d0, ws + L.enc3p[0], 0, 32, 0);
        add_src(d0, ws + L.enc3p[1], 0, 32, 0);
        d0.out_spk = ws + L.dec0p;
        CK(fldr_conv2d_spk_rows(&d0, rows.dec0, s));
        fldr_spk_conv_desc d1 = spk_desc(m->dec1, 1, Hp / 4, Wp / 4, 1);
        add_src(d1, ws + L.dec0p, 0, 64, 1);
        add_src(d1, ws + L.enc2p, 0, 32, 0);
        d1.out_spk = ws + L.dec1p;
        CK(fldr_conv2d_spk_rows(&d1, rows.dec1, s));
        // dec2 + dec3 + softmax / T + blend (fldr_hip.dec23_synth), in the output form asked for
        const float* cand[6] = {w0, w1, it0, it1, I0, I1};
        const int64_t cb[6] = {0, 0, 0, 0, 0, 0};
        const int64_t cc[6] = {HW, HW, HW, HW, 2 * HW, 2 * HW};
        if (io->output == FLDR_MODEL_OUT_U10_PLANAR) {                   // the 8-bit output's split: fused for even W, L.f64 + a rounding pass for odd W
            uint16_t* o16 = (uint16_t*)io->out[k];
            if (L.W & 1) {
                double* f64 = (double*)(ws + L.f64);
                CK(fldr_dec23_synth_rows(ws + L.dec1p, ws + L.enc1p, m->w2pack, m->bias2, m->w3m, m->bias3, cand, cb, cc, t, m->T, f64, nullptr, nullptr,
                                         0, 0, 1, Hp, Wp, rows.dec23, s));
                CK(fldr_quantize_u16(f64, 1, o16, U10_MAX, 1, L.H, L.W, Hp, Wp, s));
            } else {
                CK(fldr_dec23_synth_u16_rows(ws + L.dec1p, ws + L.enc1p, m->w2pack, m->bias2, m->w3m, m->bias3, cand, cb, cc, t, m->T, o16, U10_MAX,
                                             L.H, L.W, 1, Hp, Wp, rows.dec23, s));
            }
            continue;
        }
        double* o64 = nullptr;
        uint8_t* o8 = nullptr;
        uint8_t* planar = io->output == FLDR_MODEL_OUT_U8_PLANAR ? (uint8_t*)io->out[k] : (uint8_t*)(ws + L.u8);
        if (io->output == FLDR_MODEL_OUT_F64) o64 = (double*)io->out[k];
        else if (L.W & 1) o64 = (double*)(ws + L.f64);                   // dec23's 8-bit form needs an even width
        else o8 = planar;
        CK(fldr_dec23_synth_rows(ws + L.dec1p, ws + L.enc1p, m->w2pack, m->bias2, m->w3m, m->bias3, cand, cb, cc, t, m->T, o64, nullptr, o8,
                                 o8 ? L.H : 0, o8 ? L.W : 0, 1, Hp, Wp, rows.dec23, s));
        if (io->output != FLDR_MODEL_OUT_F64 && (L.W & 1))
            CK(fldr_frame_metrics(o64, 1, nullptr, planar, nullptr, 1, L.H, L.W, Hp, Wp, s));
        if (io->output == FLDR_MODEL_OUT_U8_INTERLEAVED)
            CK(planar_to_interleaved(planar, (uint8_t*)io->out[k], io->out_pitch, io->out_order == FLDR_MODEL_RGB, L.H, L.W, s));
    }
    return 0;
}

int validate_io(const fldr_model* m, const fldr_model_io* io) {
    if (!io) return FLDR_MODEL_E_ARG;
    if (io->batch != 1) return FLDR_MODEL_E_BATCH;
    if (io->n_t < 1 || !io->t || !io->out) return FLDR_MODEL_E_ARG;
    for (int k = 0; k < io->n_t; ++k) if (!io->out[k]) return FLDR_MODEL_E_ARG;
    if (io->output < FLDR_MODEL_OUT_F64 || io->output > FLDR_MODEL_OUT_U10_PLANAR) return FLDR_MODEL_E_ARG;
    if (io->output == FLDR_MODEL_OUT_U10_PLANAR)                          // pairs of 16-bit pixels are stored as one word
        for (int k = 0; k < io->n_t; ++k) if ((uintptr_t)io->out[k] & 3) return FLDR_MODEL_E_ARG;
    if ((unsigned)io->in_order > 1u || (unsigned)io->out_order > 1u) return FLDR_MODEL_E_ARG;
    if (io->output == FLDR_MODEL_OUT_U8_INTERLEAVED && io->out_pitch < 3ll * io->W) return FLDR_MODEL_E_ARG;
    switch (io->input) {
    case FLDR_MODEL_IN_PYRAMID:
        for (int i = 0; i <= m->S; ++i) if (!io->pyramid[i]) return FLDR_MODEL_E_ARG;
        break;
    case FLDR_MODEL_IN_U8_PLANAR:
        if (!io->frames_u8) return FLDR_MODEL_E_ARG;
        break;
    case FLDR_MODEL_IN_U10_PLANAR:
        if (!io->frames_u8 || ((uintptr_t)io->frames_u8 & 1)) return FLDR_MODEL_E_ARG;
        break;
    case FLDR_MODEL_IN_U8_INTERLEAVED:
        if (!io->frame[0] || !io->frame[1]) return FLDR_MODEL_E_ARG;
        if (io->frame_pitch[0] < 3ll * io->W || io->frame_pitch[1] < 3ll * io->W) return FLDR_MODEL_E_ARG;
        break;
    default: return FLDR_MODEL_E_ARG;
    }
    return 0;
}

}  // namespace

extern "C" FLDR_MODEL_API int fldr_model_forward(const fldr_model* m, const fldr_model_io* io, void* ws, int64_t ws_bytes, void* stream) {
    if (!m) return FLDR_MODEL_E_ARG;
    const int v = validate_io(m, io);
    if (v) return v;
    Layout L;
    const int p = plan(m->S, io->H, io->W, io->n_t, L);
    if (p) return p;
    if (!ws || ((uintptr_t)ws & (ALIGN - 1))) return FLDR_MODEL_E_ARG;
    if (ws_bytes < L.total) return FLDR_MODEL_E_WORKSPACE;
    // fault flags of earlier forwards, read without a synchronisation (fldr_hip.poll_status): nothing is enqueued behind a fault
    if (m->status[0] || m->status[1]) return FLDR_MODEL_E_STATUS;
    DeviceGuard g(m->device);
    if (g.rc) return g.rc;
    return enqueue(m, io, (char*)ws, L, (hipStream_t)stream);
}

extern "C" FLDR_MODEL_API int fldr_model_interpolate_host(const fldr_model* m, const uint8_t* i0, const uint8_t* i1, int H, int W, int64_t pitch,
                                                          int order, const float* t, int n_t, uint8_t* const* out) {
    if (!m || !i0 || !i1 || !t || !out || n_t < 1 || H < 2 || W < 2 || pitch < 3ll * W || (unsigned)order > 1u) return FLDR_MODEL_E_ARG;
    for (int k = 0; k < n_t; ++k) if (!out[k]) return FLDR_MODEL_E_ARG;
    const int64_t wsb = fldr_model_workspace_bytes(m, H, W, n_t);
    if (wsb < 0) return (int)wsb;
    DeviceGuard g(m->device);
    if (g.rc) return g.rc;
    const int64_t row = 3ll * W, fb = align_up(row * H);
    char* mem = nullptr;
    const int64_t total = wsb + 2 * fb + (int64_t)n_t * fb + align_up((int64_t)n_t * 4);
    if (hipMalloc((void**)&mem, (size_t)total) != hipSuccess) { (void)hipGetLastError(); return FLDR_MODEL_E_DEVICE; }
    hipStream_t s = nullptr;
    int rc = 0;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { (void)hipFree(mem); return FLDR_MODEL_E_DEVICE; }
    char* ws = mem;
    uint8_t* f0 = (uint8_t*)(mem + wsb);
    uint8_t* f1 = f0 + fb;
    uint8_t* o = f1 + fb;
    float* td = (float*)(o + (int64_t)n_t * fb);
    std::vector<void*> outs(n_t);
    for (int k = 0; k < n_t; ++k) outs[k] = o + (int64_t)k * fb;
    hipError_t e = hipMemcpy2DAsync(f0, row, i0, pitch, row, H, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpy2DAsync(f1, row, i1, pitch, row, H, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(td, t, (size_t)n_t * 4, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) rc = (int)e;
    if (!rc) {
        fldr_model_io io;
        memset(&io, 0, sizeof(io));
        io.batch = 1; io.H = H; io.W = W; io.input = FLDR_MODEL_IN_U8_INTERLEAVED;
        io.frame[0] = f0; io.frame[1] = f1; io.frame_pitch[0] = io.frame_pitch[1] = row; io.in_order = order;
        io.n_t = n_t; io.t = td; io.output = FLDR_MODEL_OUT_U8_INTERLEAVED; io.out_order = order; io.out = outs.data(); io.out_pitch = row;
        rc = fldr_model_forward(m, &io, ws, wsb, s);
    }
    for (int k = 0; k < n_t && !rc; ++k) {
        e = hipMemcpy2DAsync(out[k], pitch, outs[k], row, row, H, hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) rc = (int)e;
    }
    e = hipStreamSynchronize(s);
    if (!rc && e != hipSuccess) rc = (int)e;
    (void)hipStreamDestroy(s);
    (void)hipFree(mem);
    if (!rc && (m->status[0] || m->status[1])) rc = FLDR_MODEL_E_STATUS;     // a fault of this very forward: the frames are not to be trusted
    return rc;
}
