// The fp16-split arithmetic that conv_f16s.hip and refine.hip share.  Forced inline: every call compiles to the code the kernels used to spell
// out (scripts/isa_same.py, profiles/conv_common_isa.txt).  fp16-split arithmetic (the why: conv_f16s.hip's header): x = hi + lo / 2048;
// sum x*w ~= sum hi*hi + (sum hi*lo + sum lo*hi) / 2048 with two fp32 accumulators per tile, main and low.
#pragma once
#include "pmn_common.hpp"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));

#define PMN_F16S_LO_SCALE 2048.0f

// ---- split --------------------------------------------------------------------------------------------------------------------
// hi = fp16(x) rounds to nearest even; x - hi is exact in fp32; lo = fp16((x - hi) * 2048).  On 2-vectors (v_cvt_pk / v_pk_mul).
__device__ __forceinline__ f16x2_t f16s_hi2(const f32x2_t x) { return __builtin_convertvector(x, f16x2_t); }
__device__ __forceinline__ f16x2_t f16s_lo2(const f32x2_t x, const f16x2_t hi) {
    return __builtin_convertvector((x - __builtin_convertvector(hi, f32x2_t)) * PMN_F16S_LO_SCALE, f16x2_t);
}
// four values: both hi halves first (the order the kernels were measured with)
__device__ __forceinline__ void f16s_split4(const float x0, const float x1, const float x2, const float x3, f16x4& hi, f16x4& lo) {
    const f32x2_t x01 = {x0, x1}, x23 = {x2, x3};
    const f16x2_t h01 = f16s_hi2(x01), h23 = f16s_hi2(x23);
    const f16x2_t l01 = f16s_lo2(x01, h01), l23 = f16s_lo2(x23, h23);
    hi = f16x4{h01[0], h01[1], h23[0], h23[1]};
    lo = f16x4{l01[0], l01[1], l23[0], l23[1]};
}
__device__ __forceinline__ void f16s_split4(const f32x4_t x, f16x4& hi, f16x4& lo) { f16s_split4(x[0], x[1], x[2], x[3], hi, lo); }
__device__ __forceinline__ void f16s_split4(const float4 x, f16x4& hi, f16x4& lo) { f16s_split4(x.x, x.y, x.z, x.w, hi, lo); }

// ---- epilogue: main + low / 2048 + shift (folded BatchNorm / bias), in this order; ReLU ----------------------------------------
__device__ __forceinline__ f32x4_t f16s_epilogue(const f32x4_t m, const f32x4_t l, const f32x4_t shift) {
    return m + l * (1.0f / PMN_F16S_LO_SCALE) + shift;
}
__device__ __forceinline__ float f16s_epilogue(const float m, const float l, const float shift) {
    return m + l * (1.0f / PMN_F16S_LO_SCALE) + shift;
}
__device__ __forceinline__ f32x4_t f16s_relu(const f32x4_t v) { return __builtin_elementwise_max(v, f32x4_t{0.f, 0.f, 0.f, 0.f}); }
