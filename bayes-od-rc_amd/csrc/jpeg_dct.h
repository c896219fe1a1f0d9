// Device functions the JPEG decoder (jpeg_kernels.hip) and the JPEG corruption's block round trip (corrupt_kernels.hip) share:
// libjpeg's "islow" 1-D inverse transform, its descale and its YCbCr -> RGB arithmetic.  Integer arithmetic only; products and
// sums are formed in uint32 (two's complement, wrap-around defined) and read back as int32.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ int32_t jpeg_descale(uint32_t x, int s) { return (int32_t)(x + (1u << (s - 1))) >> s; }

// jidctint.c's 1-D transform (CONST_BITS = 13) on x[0..7] in place, without the descale.
__device__ __forceinline__ void jpeg_idct_1d(uint32_t x[8]) {
    uint32_t z1 = (x[2] + x[6]) * 4433u;
    const uint32_t t2 = z1 - x[6] * 15137u, t3 = z1 + x[2] * 6270u;
    const uint32_t t0 = (x[0] + x[4]) << 13, t1 = (x[0] - x[4]) << 13;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    uint32_t a = x[7], b = x[5], c = x[3], d = x[1];
    z1 = a + d;
    uint32_t z2 = b + c, z3 = a + c, z4 = b + d;
    const uint32_t z5 = (z3 + z4) * 9633u;
    a *= 2446u; b *= 16819u; c *= 25172u; d *= 12299u;
    z1 *= (uint32_t)-7373; z2 *= (uint32_t)-20995;
    z3 = z3 * (uint32_t)-16069 + z5; z4 = z4 * (uint32_t)-3196 + z5;
    a += z1 + z3; b += z2 + z4; c += z2 + z3; d += z1 + z4;
    x[0] = t10 + d; x[1] = t11 + c; x[2] = t12 + b; x[3] = t13 + a;
    x[4] = t13 - a; x[5] = t12 - b; x[6] = t11 - c; x[7] = t10 - d;
}

// jdcolor.c: one pixel from its luma sample and its chroma samples minus 128
__device__ __forceinline__ void jpeg_ycc_to_rgb(int Y, int cb, int cr, int& R, int& G, int& B) {
    R = min(max(Y + ((91881 * cr + 32768) >> 16), 0), 255);
    B = min(max(Y + ((116130 * cb + 32768) >> 16), 0), 255);
    G = min(max(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16), 0), 255);
}
