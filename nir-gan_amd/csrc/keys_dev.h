// The NDVI value and the order-preserving selection keys shared by windowstats.hip (window medians) and valpanel.hip (rgb percentiles
// and NDVI display planes): ONE statement each, so that a value is the same bits wherever and however often it is recomputed.
#pragma once
#include "common.h"

// two additions, one subtraction and one IEEE division (the library is built without fast-math): there is no multiply-add the
// compiler could contract at one call site and not at another, and contraction is switched off in the function all the same
__device__ __forceinline__ float ndvi_value(float n, float r) {
#pragma clang fp contract(off)
    return __fdiv_rn(n - r, (n + r) + 1e-6f);   // the association of pix_loss_kernel (losses.hip)
}

// 32-bit key whose unsigned order is the float order: sign bit flipped for positive floats, all bits for negative ones
__device__ __forceinline__ unsigned key_of(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float value_of(unsigned key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}
