"""The weight prepacks of libfldr_hip on seeded weights -> sha256 of the whole packed buffer, header included
(tests/test_gpu_conv_ops.py: test_prepack_bytes_are_the_recorded_ones).  Every call packs a FRESH tensor through the C entry point into a
buffer prefilled with a sentinel, so neither the wrappers' cache on the weight object nor a float the prepack leaves unwritten can
stand in for a packed byte.

Weights: numpy default_rng(seed).standard_normal / sqrt(fan-in) as float32; `zero`: all zeros (the scale = 1 branch); `spike`: the
weights of tests/conv_cases.py's spike kind (everything / 32, ONE weight at 1e3 / (32 sqrt(fan-in))), so the scale is not 1.

Shapes: the smallest that reach every branch of the layout code.  3x3 (split and spk): every nmt / groups branch of the cout
geometry, a partial input chunk (cin % 16) and a partial output block (cout % 16); 64 and 96 outputs reach the spk R32 section.
Stride 2: (32, 16) has a DMA section, (32, 12) none (cin % 8), (32, 64) the largest one, (64, 33) two 32-channel blocks, (17, 112) the
widest input.  dec23, dec3: their one shape.  ringrow (test build hook): 48 and 32 outputs of 32 inputs, its two block counts."""
import ctypes
import hashlib
import math

import numpy as np
import torch

S1_SHAPES = [(16, 3), (17, 16), (48, 17), (64, 40), (96, 100)]
S2_SHAPES = [(16, 7), (32, 16), (32, 12), (32, 64), (64, 33), (17, 112)]
RINGROW_SHAPES = [(48, 32), (32, 32)]
SENTINEL = -12345.678


def weight(shape, seed, kind="plain"):
    n = int(np.prod(shape[1:]))
    g = np.random.default_rng(seed)
    w = (g.standard_normal(shape) / math.sqrt(n)).astype(np.float32)
    if kind == "zero":
        w[...] = 0.0
    elif kind == "spike":
        w /= np.float32(32)
        i = int(g.integers(0, w.size))
        w.reshape(-1)[i] = np.float32(1e3 / (32 * math.sqrt(n))) * (1.0 if w.reshape(-1)[i] >= 0 else -1.0)
    return torch.from_numpy(w)


def _digest(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def _pack(hip, L, name, w, n_floats, dims, dev, extra=()):
    """L.<name>(weight, [extra...,] wpack, dims..., stream) into a sentinel-filled buffer of n_floats -> the buffer."""
    assert n_floats > 0, (name, n_floats)
    wd = w.to(dev).contiguous()
    wp = torch.full((int(n_floats),), SENTINEL, device=dev, dtype=torch.float32)
    ptrs = [ctypes.c_void_p(wd.data_ptr())] + [ctypes.c_void_p(e.data_ptr()) for e in extra] + [ctypes.c_void_p(wp.data_ptr())]
    rc = getattr(L, name)(*ptrs, *dims, hip._stream())
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    return wp


def _conv(hip, L, fam, cout, cin, seed, kind, dev):
    k = 4 if fam == "s2" else 3
    w = weight((cout, cin, k, k), seed, kind)
    n = getattr(L, "fldr_conv_%s_prepack_size" % fam)(cout, cin)
    return _pack(hip, L, "fldr_conv_%s_prepack" % fam, w, n, (cout, cin), dev)


def product_digests(hip, dev):
    """{case id: sha256} of every prepack of the product library."""
    L = hip.lib()
    out = {}
    seed = 1000
    for fam, shapes in (("split", S1_SHAPES), ("spk", S1_SHAPES), ("s2", S2_SHAPES)):
        for cout, cin in shapes:
            seed += 1
            out["%s %d<-%d" % (fam, cout, cin)] = _digest(_conv(hip, L, fam, cout, cin, seed, "plain", dev))
        for kind, (cout, cin) in (("zero", shapes[1]), ("spike", shapes[3])):
            seed += 1
            out["%s %d<-%d %s" % (fam, cout, cin, kind)] = _digest(_conv(hip, L, fam, cout, cin, seed, kind, dev))
    for kind in ("plain", "zero", "spike"):
        seed += 1
        out["dec23 %s" % kind] = _digest(_pack(hip, L, "fldr_dec23_prepack", weight((16, 48, 3, 3), seed, kind), L.fldr_dec23_prepack_size(), (), dev))
        seed += 1
        out["dec3_spk %s" % kind] = _digest(_pack(hip, L, "fldr_dec3_prepack_spk", weight((6, 16, 3, 3), seed, kind), L.fldr_dec3_prepack_spk_size(), (), dev))
    out["dec3 plain"] = _digest(_pack(hip, L, "fldr_dec3_prepack", weight((6, 16, 3, 3), 2001, "plain"), 1536, (), dev))
    return out


def ringrow_digests(hip, L, dev):
    """{case id: sha256} of fldr_debug_ringrow_prepack (L: the test build, inside hip.test_hooks())."""
    L.fldr_debug_ringrow_pack_floats.restype = ctypes.c_int64
    L.fldr_debug_ringrow_pack_floats.argtypes = [ctypes.c_int, ctypes.c_int]
    L.fldr_debug_ringrow_prepack.restype = ctypes.c_int
    L.fldr_debug_ringrow_prepack.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 2 + [ctypes.c_void_p]
    out = {}
    seed = 3000
    for kind, (cout, cin) in [("plain", s) for s in RINGROW_SHAPES] + [("zero", RINGROW_SHAPES[0]), ("spike", RINGROW_SHAPES[0])]:
        seed += 1
        w = weight((cout, cin, 3, 3), seed, kind)
        wpack = _pack(hip, L, "fldr_conv_spk_prepack", w, L.fldr_conv_spk_prepack_size(cout, cin), (cout, cin), dev)     # (its header holds the scale)
        wrow = _pack(hip, L, "fldr_debug_ringrow_prepack", w, L.fldr_debug_ringrow_pack_floats(cout, cin), (cout, cin), dev, extra=(wpack,))
        out["ringrow %d<-%d %s" % (cout, cin, kind)] = _digest(wrow)
    return out


# Recorded on an MI355X from the libraries of commit 80b93a2 ("Cadence, pulldown and probe: one tile reduce, one cycle stream, one check"),
# the last one before the prepack kernels were folded into csrc/weight_pack.h: never regenerate them from the code under test.
DIGESTS = {
    "split 16<-3": "5fea5d56485c94483654af98b0063be17a72fd8018e17b92257a2cd462fdce3d",
    "split 17<-16": "1e6af6b865bfff594f1a8c0c39f02d74ef74c09ca1bc03af695911f9616b3d61",
    "split 48<-17": "23c3197754e38c0eee4d4c0d85b4a8285413349128ed50d1a89b6c46500d45c1",
    "split 64<-40": "57612e55ea467a71bfa74356fcb882c2f39d948338756d1610218e7c996387aa",
    "split 96<-100": "1d1ec273743e4a286a2c53df69a7df34f8982e38c48d462ac7f50da0e2958960",
    "split 17<-16 zero": "229acb46ca7b61b57e093d4b4fafbb86d8e1f32e4d20a9828dd5cd67d704b43b",
    "split 64<-40 spike": "db327b7692d1b6cc6a7431331f69ffd50bdbb792d5d85e9c4f80330287b66a2f",
    "spk 16<-3": "aa702778537331784cb0ba982fdf3321016d4232825b983bcb5044fc47f17d09",
    "spk 17<-16": "4cf9070eb85c240b04d088f7969a7044f71bbb088ef71913a75a48859f4ebfc1",
    "spk 48<-17": "23c2a8ce74916e619677bb03163819dc96966885773ee0f8c043b2bcdbd1b8ee",
    "spk 64<-40": "04fe7789f88680df919a2bfa2bfc37f49ea28e3d6ffc3391b8a678adb298d1e1",
    "spk 96<-100": "25b533c62df99fc66cadf5274eedd4019ecfee83cd63ed680408021247bfc38d",
    "spk 17<-16 zero": "96cb995524900d86124050a70cf20efcd5179220f9d34a893b7c635d2ca9ef8f",
    "spk 64<-40 spike": "21e491bad027c1f6399fc6c0610ed5a23f906cf1983019f674daa0db680e2a18",
    "s2 16<-7": "d328f48e110e318a5e73b25e8105f774baa9fd2072894354be9e8d0d45b9af7c",
    "s2 32<-16": "93919994c3cee0e30861b2432ad6227a439ebaa5d153b22b129c8ca31f839181",
    "s2 32<-12": "f5e642eed9bd68d373d978b3782b5c3afa5de9520bd41d6b0fd886bb8896feb9",
    "s2 32<-64": "530005c711b98ecfad13f3c969624e9478d65b2373dc5df58de9a9a509980c55",
    "s2 64<-33": "4001b70a46e20bebb4eed6113f20bff7f29bc7ddbd9f5a7afee202fb18990e7a",
    "s2 17<-112": "cf3a77f896fd76f303e20346e8e36d635f8003896fcd47b531fc7213b60b36f7",
    "s2 32<-16 zero": "7081afd8518dfd45c9ed9143bcb3a0366a243c4ffcce0dffff520e86acbdc455",
    "s2 32<-64 spike": "f86dc9a01bf52e4834f3a6341e9a82029333d2c0d4395d06949a29c6515e2556",
    "dec23 plain": "24b81369c782d7254f77ae607436de64b24040755aac7eb04d4edc8f1f2f0257",
    "dec3_spk plain": "bbb46df2cd4fcdd490aaba1aa440373ce9f799f4b38ef5b664970dde551c9dd6",
    "dec23 zero": "14e4f2b5590c93bb3e0bd535e68d2ddc51260859a649131c34ffa421f2dea677",
    "dec3_spk zero": "8e77598bffbc58176840f918ba84202df68a09c830494ad40fcd3d9cd87a313d",
    "dec23 spike": "1bdd729ed6ad847ee697c1214bf105a5c28b7049024e7b6c14e056342701cea3",
    "dec3_spk spike": "f3cc9a9ab01863970d2c96c143653dadf9f576236b14a34d64f783a36a57c653",
    "dec3 plain": "b48c5d16802485b0321ec50212f73eff78fe9eb823fa3a2786088c66632c3866",
    "ringrow 48<-32 plain": "7c5c1a04a784dbd5e1c8f552599bc2b0e2a1f3700707d5b5163a522163305195",
    "ringrow 32<-32 plain": "ae0929cd3924b8e1a7e5a027d7de04b09d719051304a702e21e3c16055dff0fb",
    "ringrow 48<-32 zero": "35295da1d5eca0b6db3168c0a64a2d61ed3ae8ca283dd4aa6116aa04703dcb60",
    "ringrow 48<-32 spike": "006cbcc942fb0f3d01e93489a5a00fe69b94bb9b5928cf2538b3185e8e3aefec",
}
