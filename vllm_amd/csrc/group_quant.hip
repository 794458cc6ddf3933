// Per-token-group fp8 (OCP e4m3fn) quantisation for gfx950: the activation quantiser of the
// block-scaled linear path (DeepSeek-V3 style, 1 x g activation scales).
//
//   for every group of g consecutive elements of a row of input[num_tokens, hidden]:
//     amax = max(eps, max |float(x)|)
//     s    = amax / fp8_max                  (ue8m0: rounded up to a power of two)
//     q    = e4m3( clamp(float(x) / s, fp8_min, fp8_max) )
//
// restating csrc/quantization/fp8/per_token_group_quant.cu:43, 91-109 of the reference.
//
// Work split: the input is contiguous and hidden % g == 0, so the groups of the whole tensor
// are one flat sequence: group G starts at element G g.  A lane owns 8 consecutive elements
// (16 B of bf16 / f16, 32 B of f32), a group takes g / 8 lanes of a P-lane segment (P = the
// next power of two, at least 8), a wave quantises 64 / P groups per step -- 4 for g = 128 --
// and the waves walk the groups with a grid stride.  A group never leaves its wave:
//   * every element is read from global memory once and stays in registers between the
//     amax pass and the quantise pass;
//   * the maximum is reduced with DPP inside the 16-lane row (quad_perm, row_half_mirror,
//     row_mirror); only g > 128 crosses rows (two more wave shuffles).  No LDS, no barrier;
//   * x / s is the correctly rounded quotient: Markstein's FMA sequence on the reciprocal
//     (common.cuh div_rn), and a true division for the wave in the rare step whose
//     operands could make the residual inexact (|x| or s below 2^-100);
//   * codes are packed four at a time with v_cvt_pk_fp8_f32 and stored 8 B per lane.
// Scales go out through two element strides, which serves the row-major [T, H/g] layout and
// the reference's "column-major" one (tokens contiguous).
#include "quant_helpers.cuh"

namespace va {

constexpr int GQ_WAVES = 4;

template <typename T, int P>
__global__ __launch_bounds__(GQ_WAVES * 64) void group_quant_kernel(
    uint8_t* __restrict__ out_q, float* __restrict__ out_s, const T* __restrict__ in,
    int64_t num_groups, int group_size, int groups_per_row, float eps, float qmin, float qmax,
    int ue8m0, int64_t s_stride_token, int64_t s_stride_group) {
  constexpr int SEGS = 64 / P;                       // groups per wave and step
  const int lane = threadIdx.x & 63;
  const int l = lane & (P - 1), seg = lane / P;
  const bool has = l < (group_size >> 3);            // lanes of the segment that hold data
  const int64_t wave = (int64_t)blockIdx.x * GQ_WAVES + (threadIdx.x >> 6);
  const int64_t step = (int64_t)gridDim.x * GQ_WAVES * SEGS;

  // the loop bounds are wave-uniform: every DPP below runs with all 64 lanes enabled
  for (int64_t g0 = wave * SEGS; g0 < num_groups; g0 += step) {
    const int64_t grp = g0 + seg;
    const bool ok = has && grp < num_groups;
    const int64_t e = ok ? grp * group_size + l * 8 : 0;   // idle lanes re-read element 0
    float f[8];
    load8(in + e, f);

    float m = 0.f;
    uint32_t lo = 0xffffffffu;                       // smallest non-zero |x| bits, minus one
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      m = fmaxf(m, fabsf(f[j]));
      if constexpr (!__is_same(T, f16_t)) {          // an f16 is never below 2^-24
        const uint32_t b = (__float_as_uint(f[j]) & 0x7fffffffu) - 1u;
        lo = b < lo ? b : lo;
      }
    }
    m = seg_max<P>(ok ? m : 0.f);
    m = fmaxf(m, eps);
    float s = m / qmax;
    if (ue8m0) {
      // the smallest power of two >= max(|s|, 1e-10): a non-zero mantissa carries into the
      // exponent
      const uint32_t b = __float_as_uint(fmaxf(fabsf(s), 1e-10f));
      s = __uint_as_float((b + 0x007fffffu) & 0x7f800000u);
    }
    if (ok && l == 0) {
      const int64_t token = grp / groups_per_row;
      const int64_t gi = grp - token * groups_per_row;
      out_s[token * s_stride_token + gi * s_stride_group] = s;
    }

    const uint2 q = group_quant8(f, s, lo, qmin, qmax);
    if (ok) *reinterpret_cast<uint2*>(out_q + e) = q;
  }
}

template <typename T>
static void launch_group_quant(void* out_q, float* out_s, const void* in, int64_t num_groups,
                               int group_size, int groups_per_row, float eps, float qmin,
                               float qmax, int ue8m0, int64_t sst, int64_t ssg, hipStream_t st) {
  const int lanes = group_size / 8;
  const int p = lanes <= 8 ? 8 : lanes <= 16 ? 16 : lanes <= 32 ? 32 : 64;
  // one step of a workgroup covers 4 * 64 / P groups; short inputs get one step per workgroup
  // (1 x 7168, g = 128: 4 workgroups), long ones at most 8 workgroups per CU and a grid stride
  const int64_t per_wg = GQ_WAVES * (64 / p);
  int64_t grid = (num_groups + per_wg - 1) / per_wg;
  if (grid > 256 * 8) grid = 256 * 8;
#define GQ(P)                                                                                    \
  hipLaunchKernelGGL((group_quant_kernel<T, P>), dim3((unsigned)grid), dim3(GQ_WAVES * 64), 0,  \
                     st, (uint8_t*)out_q, out_s, (const T*)in, num_groups, group_size,           \
                     groups_per_row, eps, qmin, qmax, ue8m0, sst, ssg)
  if (p == 8) GQ(8); else if (p == 16) GQ(16); else if (p == 32) GQ(32); else GQ(64);
#undef GQ
}

}  // namespace va

using namespace va;

extern "C" int vllm_amd_per_token_group_fp8_quant(void* out_q, float* out_s, const void* input,
                                                  int64_t num_tokens, int hidden_size,
                                                  int group_size, float eps, float fp8_min,
                                                  float fp8_max, int scale_ue8m0,
                                                  int64_t s_stride_token, int64_t s_stride_group,
                                                  int dtype, void* stream) {
  const char* op = "per_token_group_fp8_quant";
  VA_REQUIRE(num_tokens >= 0 && hidden_size >= 0, VLLM_AMD_EINVAL, "%s: bad shape", op);
  VA_REQUIRE(group_size > 0 && hidden_size % group_size == 0, VLLM_AMD_EINVAL,
             "%s: hidden size %d is not a multiple of the group size %d", op, hidden_size,
             group_size);
  VA_REQUIRE(group_size % 8 == 0 && group_size <= 512, VLLM_AMD_EUNSUPPORTED,
             "%s: group size %d must be a multiple of 8, at most 512", op, group_size);
  VA_REQUIRE(dtype == VLLM_AMD_F32 || dtype == VLLM_AMD_F16 || dtype == VLLM_AMD_BF16,
             VLLM_AMD_EUNSUPPORTED, "%s: unsupported dtype %d", op, dtype);
  if (num_tokens == 0 || hidden_size == 0) return VLLM_AMD_OK;
  VA_REQUIRE(out_q && out_s && input, VLLM_AMD_EINVAL, "%s: null pointer", op);
  VA_REQUIRE((((uintptr_t)input) & 15) == 0 && (((uintptr_t)out_q) & 7) == 0,
             VLLM_AMD_EUNSUPPORTED, "%s: input must be 16-byte and output 8-byte aligned", op);
  const int gpr = hidden_size / group_size;
  const int64_t ng = num_tokens * gpr;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == VLLM_AMD_F32)
    launch_group_quant<float>(out_q, out_s, input, ng, group_size, gpr, eps, fp8_min, fp8_max,
                              scale_ue8m0, s_stride_token, s_stride_group, st);
  else if (dtype == VLLM_AMD_F16)
    launch_group_quant<f16_t>(out_q, out_s, input, ng, group_size, gpr, eps, fp8_min, fp8_max,
                              scale_ue8m0, s_stride_token, s_stride_group, st);
  else
    launch_group_quant<bf16_t>(out_q, out_s, input, ng, group_size, gpr, eps, fp8_min, fp8_max,
                               scale_ue8m0, s_stride_token, s_stride_group, st);
  VA_LAUNCH_CHECK("per_token_group_fp8_quant launch");
  return VLLM_AMD_OK;
}
