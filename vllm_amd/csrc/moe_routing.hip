// MoE routing for gfx950: softmax top-k (fused_topk / _moe_C::topk_softmax, the reference's
// csrc/moe/topk_softmax_kernels.cu) and grouped top-k (the reference's torch grouped_topk,
// vllm/model_executor/layers/fused_moe/fused_moe.py:920-975), each ONE launch of one kernel.
//
// Work split.  One wavefront per token, four tokens per 256-thread workgroup, no LDS and no barrier.
// Lane l holds the V consecutive experts [l V, l V + V) in registers, V = the power of two >= ceil(E / 64)
// (E <= 1024: V <= 16); experts past E hold -inf.  The row of logits is read once, with 16-byte loads where
// the row's address allows, and converted from fp32 / bf16 / f16 on load.
//
// Cross-lane work is a butterfly all-reduce whose first four levels are DPP modifiers on the VALU
// instruction (quad_perm xor 1, xor 2, row_half_mirror, row_mirror: after level i every aligned block of
// 2^i lanes agrees, so a mirror inside the next block meets the other half) and whose last two levels
// (16, 32) go through ds_bpermute (__shfl_xor).  Softmax max / sum use all six levels.
//
// Grouped mode.  sel = score (+ bias); a group's score is the sum of its two largest sel with a bias, its
// largest sel without.  When a group covers 2^s whole lanes (DeepSeek-V3: 256 experts, V 4, 8 groups of
// 8 lanes) the first s butterfly levels ARE the segmented reduction, every group at once: each lane
// merges its own top-2 with its partner's.  Otherwise (160 experts in 8 groups of 20) the groups are
// reduced one after the other, each lane offering only its members of the group, and lane g keeps group
// g's score (at most 64 groups on this path).  Either way one lane per group then holds the group's key,
// topk_group rounds of wave arg-max pick the surviving groups into a 64-bit mask, and an expert of a
// group outside the mask leaves the candidate set.
//
// Top-k.  Every candidate has a 64-bit key: the fp32 selecting score mapped to an unsigned that orders
// like the float (NaNs included: the order is total) in the high word, ~expert index in the low word.
// The larger key is the larger score, then the lower expert index; 0 is "not a candidate".  A lane keeps
// the maximum of its V keys; a round is one wave maximum of those, after which the winner's lane clears
// that key and lane k keeps round k's id and the winner's UNBIASED score (one v_readlane).  Groups are
// picked the same way (ties to the lower group).  So ids come out in descending order of the selecting
// score, distinct and inside [0, E) whatever the logits hold.  Renormalisation is one more wave sum and
// an IEEE division; lanes 0 .. topk-1 store weight, id and token_expert_indices = k * num_tokens + t.
//
// Arithmetic: expf, IEEE division, fp32 throughout (the reference's softmax of bf16 logits runs in bf16;
// here every dtype is scored in fp32).
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), the same for the three
// dtypes: V 1 / 2 / 4 / 8 / 16: 20 / 28 / 39 / 53 / 79 VGPRs, no LDS, scratch 0, occupancy 8 (6 at V 16).
// Nothing is allocated or synchronised: both entry points are graph-capturable.
#include "common.cuh"

#include <limits.h>
#include <math.h>

namespace va {

constexpr int RT_WAVES = 4;             // tokens per workgroup
constexpr int RT_MAX_EXPERTS = 1024;    // 64 lanes x V 16
constexpr int RT_MAX_TOPK = 64;         // lane k keeps result k

enum { RT_PLAIN = 0, RT_GROUP_LANES = 1, RT_GROUP_MASKED = 2 };

struct RouteParams {
  float* weights;            // [T, topk]
  void* ids;                 // [T, topk] int32 or int64
  int32_t* token_expert;     // [T, topk] or null
  const void* gating;        // [T, E], row stride `stride` elements
  const float* bias;         // [E] or null
  int64_t stride;
  int num_tokens, E, topk;
  int mode;                  // RT_*
  int G, topk_group, gs;     // groups, groups kept, experts per group
  int lpg_log2;              // RT_GROUP_LANES: log2(lanes per group)
  int sigmoid, renorm, ids64;
  int vec_gating, vec_bias;  // 16-byte (or V-element) loads are aligned
};

// ---- butterfly levels -------------------------------------------------------------------------
template <int LEVEL> __device__ __forceinline__ uint32_t bfly(uint32_t v) {
  if constexpr (LEVEL == 0) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
  else if constexpr (LEVEL == 1) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
  else if constexpr (LEVEL == 2) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true);  // row_half_mirror
  else if constexpr (LEVEL == 3) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true);  // row_mirror
  else return (uint32_t)__shfl_xor((int)v, 1 << LEVEL, 64);
}
template <int LEVEL> __device__ __forceinline__ float bfly(float v) {
  return __uint_as_float(bfly<LEVEL>(__float_as_uint(v)));
}
template <int LEVEL> __device__ __forceinline__ uint64_t bfly(uint64_t v) {
  return ((uint64_t)bfly<LEVEL>((uint32_t)(v >> 32)) << 32) | bfly<LEVEL>((uint32_t)v);
}

__device__ __forceinline__ float rt_wave_max(float v) {
  static_for<6>([&](auto l) { v = fmaxf(v, bfly<decltype(l)::value>(v)); });
  return v;
}
__device__ __forceinline__ float rt_wave_sum(float v) {
  static_for<6>([&](auto l) { v += bfly<decltype(l)::value>(v); });
  return v;
}
__device__ __forceinline__ uint64_t rt_wave_max(uint64_t v) {
  static_for<6>([&](auto l) {
    const uint64_t o = bfly<decltype(l)::value>(v);
    v = o > v ? o : v;
  });
  return v;
}

// the two largest of a multiset, as a pair (a1 >= a2)
struct Top2 { float a1, a2; };
__device__ __forceinline__ void top2_push(Top2& t, float v) {
  t.a2 = fmaxf(t.a2, fminf(t.a1, v));
  t.a1 = fmaxf(t.a1, v);
}
template <int LEVEL> __device__ __forceinline__ void top2_merge(Top2& t) {
  const float b1 = bfly<LEVEL>(t.a1), b2 = bfly<LEVEL>(t.a2);
  const float lo = fminf(t.a1, b1);
  t.a1 = fmaxf(t.a1, b1);
  t.a2 = fmaxf(lo, fmaxf(t.a2, b2));
}

// ---- keys ---------------------------------------------------------------------------------------
// float -> unsigned with the same order (-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN)
__device__ __forceinline__ uint32_t rt_ordered(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
// never 0: the low word is at least 0xffffffff - 1023
__device__ __forceinline__ uint64_t rt_key(float v, int index) {
  return ((uint64_t)rt_ordered(v) << 32) | (uint32_t)(0xffffffffu - (uint32_t)index);
}
__device__ __forceinline__ int rt_key_index(uint64_t key) {
  return __builtin_amdgcn_readfirstlane((int)(0xffffffffu - (uint32_t)key));
}

// ---- loads ----------------------------------------------------------------------------------------
// V consecutive elements from p[base ..], bounded by n; `fill` past the end
template <typename T, int V>
__device__ __forceinline__ void rt_load(const T* __restrict__ p, int base, int n, bool aligned, float fill,
                                        float (&x)[V]) {
  constexpr int C = V * (int)sizeof(T) > 16 ? 16 / (int)sizeof(T) : V;   // elements per load
  if (aligned && base + V <= n) {
#pragma unroll
    for (int c = 0; c < V / C; ++c) {
      const Vec<T, C> v = *reinterpret_cast<const Vec<T, C>*>(p + base + c * C);
#pragma unroll
      for (int j = 0; j < C; ++j) x[c * C + j] = to_f32(v.v[j]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) x[j] = base + j < n ? to_f32(p[base + j]) : fill;
  }
}

// ---- the kernel -----------------------------------------------------------------------------------
template <typename T, int V>
__global__ __launch_bounds__(RT_WAVES * 64) void moe_route_kernel(const RouteParams p) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * RT_WAVES + (threadIdx.x >> 6);
  if (t >= p.num_tokens) return;   // wave-uniform; the kernel has no barrier
  const int E = p.E, base = lane * V;
  const float ninf = -INFINITY;

  float sc[V];   // logits, then the unbiased scores
  rt_load<T, V>((const T*)p.gating + (int64_t)t * p.stride, base, E, p.vec_gating != 0, ninf, sc);
  if (p.sigmoid) {
#pragma unroll
    for (int j = 0; j < V; ++j) sc[j] = 1.0f / (1.0f + expf(-sc[j]));   // padding: 1 / (1 + inf) = 0
  } else {
    float m = sc[0];
#pragma unroll
    for (int j = 1; j < V; ++j) m = fmaxf(m, sc[j]);
    m = rt_wave_max(m);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      sc[j] = expf(sc[j] - m);   // padding: exp(-inf) = 0
      s += sc[j];
    }
    s = rt_wave_sum(s);
#pragma unroll
    for (int j = 0; j < V; ++j) sc[j] = sc[j] / s;
  }

  float sel[V];   // selecting scores
  if (p.bias) {
    rt_load<float, V>(p.bias, base, E, p.vec_bias != 0, 0.f, sel);
#pragma unroll
    for (int j = 0; j < V; ++j) sel[j] += sc[j];
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) sel[j] = sc[j];
  }

  // which of this lane's experts are candidates: bit j
  uint32_t cand = 0;
#pragma unroll
  for (int j = 0; j < V; ++j) cand |= (base + j < E ? 1u : 0u) << j;

  if (p.mode != RT_PLAIN) {
    const bool top2 = p.bias != nullptr;
    int my_group;        // the group whose key this lane offers, -1 for none
    float gscore = ninf;
    int grp[V];          // group of each expert held here
    if (p.mode == RT_GROUP_LANES) {
      const int g = lane >> p.lpg_log2;
      Top2 tt = {ninf, ninf};
#pragma unroll
      for (int j = 0; j < V; ++j) {
        grp[j] = g;
        top2_push(tt, sel[j]);
      }
      static_for<6>([&](auto l) {
        if (decltype(l)::value < p.lpg_log2) top2_merge<decltype(l)::value>(tt);
      });
      gscore = top2 ? tt.a1 + tt.a2 : tt.a1;
      my_group = ((lane & ((1 << p.lpg_log2) - 1)) == 0 && g < p.G) ? g : -1;
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) grp[j] = (base + j) / p.gs;
      for (int g = 0; g < p.G; ++g) {
        Top2 tt = {ninf, ninf};
#pragma unroll
        for (int j = 0; j < V; ++j)
          if (grp[j] == g) top2_push(tt, sel[j]);
        static_for<6>([&](auto l) { top2_merge<decltype(l)::value>(tt); });
        if (lane == g) gscore = top2 ? tt.a1 + tt.a2 : tt.a1;
      }
      my_group = lane < p.G ? lane : -1;
    }
    uint64_t gkey = my_group >= 0 ? rt_key(gscore, my_group) : 0ull;
    uint64_t alive = 0;
    for (int r = 0; r < p.topk_group; ++r) {
      const int g = rt_key_index(rt_wave_max(gkey)) & 63;
      alive |= 1ull << g;
      if (my_group == g) gkey = 0;
    }
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (grp[j] >= p.G || !((alive >> (grp[j] & 63)) & 1)) cand &= ~(1u << j);
  }

  uint64_t key[V];
  uint64_t best = 0;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    key[j] = ((cand >> j) & 1) ? rt_key(sel[j], base + j) : 0ull;
    best = key[j] > best ? key[j] : best;
  }

  float w = 0.f;
  int id = 0;
  for (int k = 0; k < p.topk; ++k) {
    int idx = rt_key_index(rt_wave_max(best));
    idx = idx < E ? idx : E - 1;   // unreachable while topk candidates exist (checked on the host)
    const int wl = idx / V, wj = idx % V;
    float s = sc[0];
#pragma unroll
    for (int j = 1; j < V; ++j) s = wj == j ? sc[j] : s;
    const float ws = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(s), wl));
    if (lane == k) {
      w = ws;
      id = idx;
    }
    if (lane == wl) {
      best = 0;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        key[j] = wj == j ? 0ull : key[j];
        best = key[j] > best ? key[j] : best;
      }
    }
  }

  if (p.renorm) {
    const float total = rt_wave_sum(lane < p.topk ? w : 0.f);
    w = w / total;
  }
  if (lane < p.topk) {
    const int64_t o = (int64_t)t * p.topk + lane;
    p.weights[o] = w;
    if (p.ids64) ((int64_t*)p.ids)[o] = id;
    else ((int32_t*)p.ids)[o] = id;
    if (p.token_expert) p.token_expert[o] = lane * p.num_tokens + t;
  }
}

// ---- launch -----------------------------------------------------------------------------------------
template <typename T, int V>
static void launch_route_v(RouteParams p, hipStream_t st) {
  constexpr int C = V * (int)sizeof(T) > 16 ? 16 / (int)sizeof(T) : V;
  constexpr int CB = V > 4 ? 4 : V;
  p.vec_gating = ((uintptr_t)p.gating % (C * sizeof(T)) == 0 && p.stride % C == 0) ? 1 : 0;
  p.vec_bias = (p.bias && (uintptr_t)p.bias % (CB * sizeof(float)) == 0) ? 1 : 0;
  const unsigned grid = (unsigned)((p.num_tokens + RT_WAVES - 1) / RT_WAVES);
  hipLaunchKernelGGL((moe_route_kernel<T, V>), dim3(grid), dim3(RT_WAVES * 64), 0, st, p);
}

static int route_v(int E) {
  int v = 1;
  while (64 * v < E) v *= 2;
  return v;
}

template <typename T>
static void launch_route_t(const RouteParams& p, hipStream_t st) {
  switch (route_v(p.E)) {
    case 1: launch_route_v<T, 1>(p, st); break;
    case 2: launch_route_v<T, 2>(p, st); break;
    case 4: launch_route_v<T, 4>(p, st); break;
    case 8: launch_route_v<T, 8>(p, st); break;
    default: launch_route_v<T, 16>(p, st); break;
  }
}

static void launch_route(const RouteParams& p, int dtype, hipStream_t st) {
  if (dtype == VLLM_AMD_F32) launch_route_t<float>(p, st);
  else if (dtype == VLLM_AMD_F16) launch_route_t<f16_t>(p, st);
  else launch_route_t<bf16_t>(p, st);
}

// the checks both entry points share; 1 = nothing to do
static int route_common(const char* op, int64_t num_tokens, int num_experts, int topk, int64_t stride, int dtype) {
  VA_REQUIRE(num_tokens >= 0, VLLM_AMD_EINVAL, "%s: num_tokens %lld is negative", op, (long long)num_tokens);
  if (num_tokens == 0) return 1;
  VA_REQUIRE(num_experts >= 1, VLLM_AMD_EINVAL, "%s: num_experts %d < 1", op, num_experts);
  VA_REQUIRE(num_experts <= RT_MAX_EXPERTS, VLLM_AMD_EUNSUPPORTED, "%s: num_experts %d > %d", op, num_experts,
             RT_MAX_EXPERTS);
  VA_REQUIRE(topk >= 1 && topk <= num_experts && topk <= RT_MAX_TOPK, VLLM_AMD_EUNSUPPORTED,
             "%s: topk %d is outside [1, min(num_experts, %d)] for num_experts %d", op, topk, RT_MAX_TOPK, num_experts);
  VA_REQUIRE(dtype == VLLM_AMD_F32 || dtype == VLLM_AMD_F16 || dtype == VLLM_AMD_BF16, VLLM_AMD_EUNSUPPORTED,
             "%s: gating dtype %d must be float32, float16 or bfloat16", op, dtype);
  VA_REQUIRE(stride >= num_experts, VLLM_AMD_EINVAL, "%s: gating stride %lld < num_experts %d", op, (long long)stride,
             num_experts);
  VA_REQUIRE(num_tokens * topk < INT_MAX, VLLM_AMD_EUNSUPPORTED, "%s: num_tokens %lld x topk %d does not fit int32",
             op, (long long)num_tokens, topk);
  return 0;
}

}  // namespace va

using namespace va;

extern "C" int vllm_amd_topk_softmax(float* topk_weights, void* topk_ids, int32_t* token_expert_indices,
                                     const void* gating_output, int64_t num_tokens, int num_experts, int topk,
                                     int64_t gating_stride, int renormalize, int gating_dtype, int ids_int64,
                                     void* stream) {
  const char* op = "topk_softmax";
  const int rc = route_common(op, num_tokens, num_experts, topk, gating_stride, gating_dtype);
  if (rc) return rc > 0 ? 0 : rc;
  VA_REQUIRE(ids_int64 == 0 || ids_int64 == 1, VLLM_AMD_EUNSUPPORTED, "%s: ids dtype %d must be 0 (int32) or 1 (int64)", op,
             ids_int64);
  VA_REQUIRE(topk_weights && topk_ids && token_expert_indices && gating_output, VLLM_AMD_EINVAL, "%s: null pointer", op);
  RouteParams p = {};
  p.weights = topk_weights; p.ids = topk_ids; p.token_expert = token_expert_indices; p.gating = gating_output;
  p.stride = gating_stride; p.num_tokens = (int)num_tokens; p.E = num_experts; p.topk = topk;
  p.mode = RT_PLAIN; p.renorm = renormalize ? 1 : 0; p.ids64 = ids_int64;
  launch_route(p, gating_dtype, (hipStream_t)stream);
  VA_LAUNCH_CHECK("topk_softmax launch");
  return 0;
}

extern "C" int vllm_amd_grouped_topk(float* topk_weights, int32_t* topk_ids, const void* gating_output,
                                     const float* e_score_correction_bias, int64_t num_tokens, int num_experts,
                                     int topk, int num_expert_group, int topk_group, int scoring_func,
                                     int renormalize, int64_t gating_stride, int gating_dtype, void* stream) {
  const char* op = "grouped_topk";
  const int rc = route_common(op, num_tokens, num_experts, topk, gating_stride, gating_dtype);
  if (rc) return rc > 0 ? 0 : rc;
  VA_REQUIRE(num_expert_group >= 1 && num_experts % num_expert_group == 0, VLLM_AMD_EINVAL,
             "%s: num_expert_group %d does not divide num_experts %d", op, num_expert_group, num_experts);
  const int gs = num_experts / num_expert_group;
  VA_REQUIRE(topk_group >= 1 && topk_group <= num_expert_group, VLLM_AMD_EINVAL,
             "%s: topk_group %d is outside [1, num_expert_group %d]", op, topk_group, num_expert_group);
  VA_REQUIRE(topk <= topk_group * gs, VLLM_AMD_EINVAL, "%s: topk %d > topk_group %d x %d experts per group", op, topk,
             topk_group, gs);
  VA_REQUIRE(!e_score_correction_bias || gs >= 2, VLLM_AMD_EINVAL,
             "%s: e_score_correction_bias needs groups of at least 2 experts, got %d", op, gs);
  VA_REQUIRE(scoring_func == VLLM_AMD_SCORE_SOFTMAX || scoring_func == VLLM_AMD_SCORE_SIGMOID, VLLM_AMD_EUNSUPPORTED,
             "%s: unknown scoring function %d", op, scoring_func);
  VA_REQUIRE(topk_weights && topk_ids && gating_output, VLLM_AMD_EINVAL, "%s: null pointer", op);
  RouteParams p = {};
  p.weights = topk_weights; p.ids = topk_ids; p.gating = gating_output; p.bias = e_score_correction_bias;
  p.stride = gating_stride; p.num_tokens = (int)num_tokens; p.E = num_experts; p.topk = topk;
  p.G = num_expert_group; p.topk_group = topk_group; p.gs = gs;
  p.sigmoid = scoring_func == VLLM_AMD_SCORE_SIGMOID; p.renorm = renormalize ? 1 : 0;
  // a group that covers 2^s whole lanes reduces with the first s butterfly levels; anything else group by group
  const int V = route_v(num_experts), lpg = gs / V;
  if (gs % V == 0 && (lpg & (lpg - 1)) == 0) {
    p.mode = RT_GROUP_LANES;
    while ((1 << p.lpg_log2) < lpg) ++p.lpg_log2;
  } else {
    VA_REQUIRE(num_expert_group <= 64, VLLM_AMD_EUNSUPPORTED,
               "%s: num_expert_group %d > 64 with groups of %d experts, which do not cover whole lanes of %d", op,
               num_expert_group, gs, V);
    p.mode = RT_GROUP_MASKED;
  }
  launch_route(p, gating_dtype, (hipStream_t)stream);
  VA_LAUNCH_CHECK("grouped_topk launch");
  return 0;
}
