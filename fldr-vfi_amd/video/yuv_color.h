// The colour definition of libfldr_video.so, in one place for the kernels and the host: 8-bit YUV 4:2:0 <-> 8-bit BGR in integer
// fixed point (each coefficient round(c * 2^16)), so the device and the numpy oracle (tests/yuv_oracle.py) give the same bytes.
//
//   forward (BGR -> YUV), sy = 219/255 (limited) or 1 (full), sc = 224/255 or 1:
//     KYR, KYB = round(Kr sy 2^16), round(Kb sy 2^16); KYG = round(sy 2^16) - KYR - KYB
//     KUB = KVR = round(sc/2 2^16); KUR = round(-sc/2 Kr/(1-Kb) 2^16), KUG = -KUB - KUR; KVB = round(-sc/2 Kb/(1-Kr) 2^16), KVG = -KVR - KVB
//   inverse (YUV -> BGR): KY = round(2^16 / sy), KRV = round(2 (1-Kr)/sc 2^16), KBU = round(2 (1-Kb)/sc 2^16),
//     KGU = round(2 (1-Kb) Kb/Kg/sc 2^16), KGV = round(2 (1-Kr) Kr/Kg/sc 2^16)
//
// Every intermediate of the kernels fits in int32 (largest |accumulator| 2.87e8, tests/test_video_cpu.py checks all 2^24 triples).
#pragma once
#include <stdint.h>

namespace fldr_video_impl {

struct YuvCoeffs {
    int32_t kyr, kyg, kyb, kur, kug, kub, kvr, kvg, kvb;     // forward
    int32_t ky, krv, kbu, kgu, kgv;                          // inverse
    int32_t yoff;                                            // 16 (limited) or 0 (full); 64 / 0 at depth 10
};

// [matrix][range]: matrix 0 = BT.601 (Kr 0.299, Kb 0.114), 1 = BT.709 (Kr 0.2126, Kb 0.0722); range 0 = limited, 1 = full
static const YuvCoeffs YUV_COEFFS[2][2] = {
    {{16829, 33039, 6416, -9714, -19070, 28784, 28784, -24103, -4681, 76309, 104597, 132201, 25675, 53279, 16},
     {19595, 38470, 7471, -11058, -21710, 32768, 32768, -27439, -5329, 65536, 91881, 116130, 22553, 46802, 0}},
    {{11966, 40254, 4064, -6596, -22188, 28784, 28784, -26145, -2639, 76309, 117489, 138438, 13975, 34925, 16},
     {13933, 46871, 4732, -7509, -25259, 32768, 32768, -29763, -3005, 65536, 103206, 121609, 12276, 30679, 0}},
};

// The same table at depth 10 (code values 0 .. 1023 in 16-bit words; numpy oracle with a depth argument: tests/yuv_hd_oracle.py).  Same
// Kr / Kb, same 16 fraction bits, siting and tap weights; at depth d, sy = 219 2^(d-8) / (2^d - 1) and sc = 224 2^(d-8) / (2^d - 1) for
// limited range (Y 64 .. 940, C 64 .. 960), yoff = 16 << (d-8), the chroma centre is 128 << (d-8) = 512 and the clamps are 0 .. 2^d - 1;
// d = 8 gives the table above.  The full-range rows are the 8-bit ones (sy = sc = 1).  The int32 accumulators still fit: the largest is
// bounded by |Y - yoff| 8 KY + KBU 8 512 + 2^18 = 1.16e9 (BT.709 limited; tests/test_video10_cpu.py bounds every one by its coefficients).
static const YuvCoeffs YUV_COEFFS_10[2][2] = {
    {{16780, 32941, 6398, -9685, -19015, 28700, 28700, -24033, -4667, 76533, 104905, 132590, 25750, 53435, 64},
     {19595, 38470, 7471, -11058, -21710, 32768, 32768, -27439, -5329, 65536, 91881, 116130, 22553, 46802, 0}},
    {{11931, 40136, 4052, -6576, -22124, 28700, 28700, -26068, -2632, 76533, 117835, 138846, 14017, 35027, 64},
     {13933, 46871, 4732, -7509, -25259, 32768, 32768, -29763, -3005, 65536, 103206, 121609, 12276, 30679, 0}},
};

}  // namespace fldr_video_impl
