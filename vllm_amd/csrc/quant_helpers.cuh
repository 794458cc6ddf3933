// Device helpers shared by the group quantiser (group_quant.hip), the fused activation quantisers
// (fused_quant.hip) and the MoE path (moe_block_fp8.hip).
#pragma once
#include "common.cuh"

namespace va {

template <int CTRL>
__device__ __forceinline__ float dpp_move(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}

// maximum over the P-lane segment of the lane; valid in every lane of the segment
template <int P>
__device__ __forceinline__ float seg_max(float v) {
  v = fmaxf(v, dpp_move<0xB1>(v));    // quad_perm [1,0,3,2]
  v = fmaxf(v, dpp_move<0x4E>(v));    // quad_perm [2,3,0,1]
  v = fmaxf(v, dpp_move<0x141>(v));   // row_half_mirror: the other quad of the 8 lanes
  if constexpr (P >= 16) v = fmaxf(v, dpp_move<0x140>(v));   // row_mirror: the other half row
  if constexpr (P >= 32) v = fmaxf(v, __shfl_xor(v, 16, 64));
  if constexpr (P >= 64) v = fmaxf(v, __shfl_xor(v, 32, 64));
  return v;
}

template <typename T>
__device__ __forceinline__ void load8(const T* p, float (&f)[8]) {
  if constexpr (sizeof(T) == 4) {
    const float4 lo = *reinterpret_cast<const float4*>(p);
    const float4 hi = *reinterpret_cast<const float4*>(p + 4);
    f[0] = lo.x; f[1] = lo.y; f[2] = lo.z; f[3] = lo.w;
    f[4] = hi.x; f[5] = hi.y; f[6] = hi.z; f[7] = hi.w;
  } else {
    const Vec<T, 8> v = *reinterpret_cast<const Vec<T, 8>*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = to_f32(v.v[j]);
  }
}

// The group quantiser's arithmetic on the 8 values of a lane, given the group's scale s:
// q = clamp(f / s, qmin, qmax) with the correctly rounded quotient (Markstein's FMA sequence on
// the reciprocal, common.cuh div_rn; a true division for the wave in the rare step whose operands
// could make the residual inexact, |x| or s below 2^-100), packed four at a time.
// lo = the smallest non-zero |x| bit pattern of the lane, minus one.
__device__ __forceinline__ uint2 group_quant8(const float (&f)[8], float s, uint32_t lo, float qmin, float qmax) {
  float q[8];
  const bool slow = lo < 0x0d800000u - 1u || !(s >= 7.9e-31f);   // 2^-100
  if (__builtin_expect(__any(slow), 0)) {
#pragma unroll
    for (int j = 0; j < 8; ++j) q[j] = f[j] / s;
  } else {
    const Divisor d(s);
#pragma unroll
    for (int j = 0; j < 8; ++j) q[j] = div_rn(f[j], d);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) q[j] = fminf(fmaxf(q[j], qmin), qmax);
  int w0 = __builtin_amdgcn_cvt_pk_fp8_f32(q[0], q[1], 0, false);
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(q[2], q[3], w0, true);
  int w1 = __builtin_amdgcn_cvt_pk_fp8_f32(q[4], q[5], 0, false);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(q[6], q[7], w1, true);
  return make_uint2((uint32_t)w0, (uint32_t)w1);
}

// silu(x) * y, rounded to T at the points the reference rounds (activation_kernels.cu:14-89)
template <typename T>
__device__ __forceinline__ float silu_mul(T x, T y) {
  const float xf = to_f32(x);
  // the hardware exp2 / rcp (each ~1 ulp): the result is rounded to T right away, and the
  // accurate expf + IEEE division made this HBM-bound op VALU-bound
  const T a = from_f32<T>(xf * __builtin_amdgcn_rcpf(1.0f + __expf(-xf)));
  return to_f32(from_f32<T>(to_f32(a) * to_f32(y)));
}

}  // namespace va
