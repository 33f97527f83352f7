// The 3-way bf16 split of include/y2_split_rule.h on the device, four values at a time, for the kernels that split an fp32
// operand in registers while they stage it into LDS (y2_train_bf16.hip, y2_conv_split.hip).  y2_wino.hip keeps its own
// restatement beside the transform it is fused into.
#pragma once
#include "y2_common.hpp"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

namespace {

__device__ __forceinline__ f32x4 bf16x4_f32(u16x4 b)
{
    const u32x4 u = __builtin_convertvector(b, u32x4) << 16;
    return __builtin_bit_cast(f32x4, u);
}

// y2_bf16_rn on four values: v_cvt_pk_bf16_f32 rounds to nearest even and quiets NaNs; a finite value never becomes an infinity
__device__ __forceinline__ u16x4 bf16_rn_x4(const f32x4 v, bool fin[4])
{
    const u32x4 bits = __builtin_bit_cast(u32x4, v);
    u16x4 h = __builtin_bit_cast(u16x4, __builtin_convertvector(v, bf16x4));
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned mag = bits[k] & 0x7fffffffu;
        fin[k] = mag < 0x7f800000u;
        if (fin[k] && mag >= 0x7f7f8000u) h[k] = (unsigned short)(((bits[k] >> 16) & 0x8000u) | 0x7f7fu);
    }
    return h;
}

// y2_split3 on four values: h + m + l == v; a non-finite v gives h = v, m = l = 0
__device__ __forceinline__ void split3_x4(const f32x4 v, u16x4 &h, u16x4 &m, u16x4 &l)
{
    bool fin[4];
    h = bf16_rn_x4(v, fin);
    f32x4 r = v - bf16x4_f32(h);
#pragma unroll
    for (int k = 0; k < 4; ++k) if (!fin[k]) r[k] = 0.f;
    m = __builtin_bit_cast(u16x4, __builtin_convertvector(r, bf16x4));
    r = r - bf16x4_f32(m);
    l = __builtin_bit_cast(u16x4, __builtin_convertvector(r, bf16x4));    // exact: the low 16 bits are zero (but for bits below 2^-133)
}

// eight staged values of one row -> PLANES 16-byte fragments at `at`, PLANE_B bytes apart per plane
template <int PLANES, int PLANE_B>
__device__ __forceinline__ void put_planes(unsigned char *at, const float (&v)[8])
{
    const f32x4 lo = {v[0], v[1], v[2], v[3]}, hi = {v[4], v[5], v[6], v[7]};
    if constexpr (PLANES == 1) {
        bool fin[4];
        const u16x4 a = bf16_rn_x4(lo, fin), b = bf16_rn_x4(hi, fin);
        *(u16x8 *)at = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
    } else {
        u16x4 h0, m0, l0, h1, m1, l1;
        split3_x4(lo, h0, m0, l0);
        split3_x4(hi, h1, m1, l1);
        *(u16x8 *)at = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
        *(u16x8 *)(at + PLANE_B) = __builtin_shufflevector(m0, m1, 0, 1, 2, 3, 4, 5, 6, 7);
        *(u16x8 *)(at + 2 * PLANE_B) = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
    }
}

}  // namespace
