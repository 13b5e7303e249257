// IEEE binary16 <-> binary32 on integer bits alone, for the host (Plan::pack_conv, plan_weights.cpp) and the device
// (head_step_kernel, head_step.hip): the step kernel re-packs a conv bit for bit as the host pack does because both run these two
// routines.  No floating-point operation, so the result does not depend on the denormal mode either side is built with.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

namespace rtod {

__host__ __device__ inline uint32_t f32_bits(float f) { uint32_t x; memcpy(&x, &f, 4); return x; }
__host__ __device__ inline float f32_from_bits(uint32_t x) { float f; memcpy(&f, &x, 4); return f; }

// round to nearest even; subnormal halves kept, values at or below 2^-25 to (signed) zero, NaN to a quiet NaN
__host__ __device__ inline uint16_t f32_to_f16_rn(float f) {
    uint32_t x = f32_bits(f);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7FFFFFFFu;
    if (x >= 0x7F800000u) return (uint16_t)(sign | (x > 0x7F800000u ? 0x7E00u : 0x7C00u));
    if (x >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);                // rounds to >= 65520 -> inf
    if (x < 0x33000001u) return (uint16_t)sign;                              // <= 2^-25 -> 0
    const int e = (int)(x >> 23) - 127;
    const uint32_t m = (x & 0x7FFFFFu) | 0x800000u;
    const int shift = (e < -14) ? (13 + (-14 - e)) : 13;                     // subnormal halves lose extra bits; <= 24 here: e >= -25
    uint32_t half_m = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1u), halfway = 1u << (shift - 1);
    if (rem > halfway || (rem == halfway && (half_m & 1u))) ++half_m;
    // subnormal: half_m alone (may carry into the first normal); normal: the carry propagates into the exponent
    const uint32_t out = (e < -14) ? half_m : (((uint32_t)(e + 15) << 10) + (half_m - 0x400u));
    return (uint16_t)(sign | out);
}

// exact: every half is a float
__host__ __device__ inline float f16_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    int e = (h >> 10) & 0x1F;
    uint32_t m = h & 0x3FFu;
    if (e == 31) return f32_from_bits(sign | (m ? 0x7FC00000u : 0x7F800000u));
    if (e == 0) {
        if (m == 0) return f32_from_bits(sign);
        const int up = __builtin_clz(m) - 21;                                // a subnormal half m * 2^-24 is a normal float: its leading bit
        m = (m << up) & 0x3FFu;                                              // becomes the implicit one
        e = 1 - up;
    }
    return f32_from_bits(sign | ((uint32_t)(e + 112) << 23) | (m << 13));
}

}  // namespace rtod
