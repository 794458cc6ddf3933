// Fused MoE experts over MXFP4 weights AND activations (w4a4) for gfx950: the three kernels behind
// fused_experts(..., use_mxfp4_w4a4=True).  MXFP4 is the OCP microscaling format: e2m1 values
// {0, .5, 1, 1.5, 2, 3, 4, 6} with a sign, two per byte (element 2 j in the low nibble of byte j), and one
// e8m0 scale byte (2^(byte - 127)) per 32 consecutive values.
//
//   mxfp4_quant                  [rows, K] bf16 / f16 -> codes [rows, K / 2], scale bytes [rows, K / 32]
//   silu_and_mul_mxfp4_quant     the same quantiser on v = T(T(silu(x)) * y), from [rows, 2 I]
//   moe_mxfp4_gemm               grouped GEMM, contract of moe_blockwise_gemm (moe_block_fp8.hip)
//
// (a) Quantiser (the reference's "even" mode, tests/quantization/reference_mxfp4.py qdq_mxfp4_torch): per
//     32-block amax = f 2^e with f in [1, 2); f >= 1.75 takes the next exponent (6 = 1.5 x 4 is the largest
//     code, so 1.75 x 4 and above would otherwise round past it); scale byte = clamp(e - 2 + 127, 0, 254),
//     0 for an all-zero block.  Both come from the fp32 bit pattern of amax: exponent field - 2, + 1 when the
//     mantissa field is >= 0.75.  x / 2^(byte - 127) is an exact ldexp; it is rounded to nearest-even onto
//     the grid in fp32 (steps .5 below 2, 1 below 4, 2 above: one v_rndne each) and saturates at 6.
//     Work split: a lane owns 8 consecutive elements (one 16-byte load, one dword of codes), the four lanes
//     of a quad own a block and meet their maxima with two DPP quad permutes; a wave covers 512 elements.
//     The fused form computes v in registers with the recipe of silu_and_mul_group_quant (quant_helpers.cuh
//     silu_mul): one read of [rows, 2 I], no 16-bit intermediate tensor.
//
// (b) Grouped GEMM.  Same contract, same work split over the sorted rows and the same epilogue as
//     moe_block_gemm_kernel: a workgroup of 8 waves serves one m-block (MT = 1 or 4 MFMA row tiles) of one
//     expert and 8 / KS strips of 16 output columns, computed transposed (A operand = weight rows), the KS
//     partial sums of a strip meet in LDS, then routed weight in fp32, one rounding, scattered row store.
//     What differs is everything between the loads and the accumulator:
//       * One v_mfma_scale_f32_16x16x128_f8f6f4 with cbsz:4 blgp:4 consumes 128 K elements = 64 bytes per
//         row.  Lane (row = lane & 15, g = lane >> 4) holds elements 32 g .. 32 g + 31 in the low four of
//         the eight operand registers: ONE 16-byte load at byte 64 kb + 16 g of the row, and exactly one MX
//         block, so the instruction's scale operands carry the e8m0 bytes of that block and the products
//         are scaled in hardware.
//       * The accumulation over K blocks therefore runs in the MFMA's C operand.  The fp8 kernel has one
//         fp32 scale pair per 128 x 128 block and folds acc = fma(partial, As Bs, acc) on the VALU per
//         block and m-tile (4 FMAs + a multiply per MFMA, and the MFMA result must leave the pipeline
//         first); here no VALU instruction touches the sums before the epilogue.  With MT 1 two
//         accumulators alternate so that consecutive MFMAs do not wait on each other.
//       * op_sel is an immediate, so the lane shifts its own byte into place: the four scale bytes of a
//         row's K block (bytes 4 kb .. 4 kb + 3) are one dword load, shifted right by 8 g, op_sel 0.
//       * A fragment is 16 bytes instead of 32, so a wave keeps UN = 8 (MT 1) / 4 (MT 4) K blocks of loads
//         in flight, twice the fp8 kernel's count: the same bytes per wave for the same VGPR budget.
//       * The KS waves of a strip take the K blocks round-robin in units of TWO blocks = one 128-byte line
//         of a weight row per wave (single blocks when the row has fewer than 2 KS of them: K 256 with
//         KS 2 would otherwise idle half of the waves).  KS keeps its meaning and its tuning key "moe_ks"
//         (8 or 2); the automatic choice is by the row length in BYTES, see launch_mxfp4_gemm.
//     Padding entries and columns past N re-read a clamped row and are never stored; expert ids outside
//     [0, E) store zeros; blocks past *num_tokens_post_padded exit.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage, bf16):
//   gemm MT 1, KS 8 / 2: 110 / 110 VGPRs, 0 AGPRs, scratch 0, LDS  8768 B, occupancy 4 waves / SIMD
//   gemm MT 4, KS 8 / 2: 156 / 154 VGPRs, 0 AGPRs, scratch 0, LDS 35072 B, occupancy 3 waves / SIMD
//   (the MFMA operands are 4-register tuples: the zero upper halves of the builtin's operands cost nothing)
//   mxfp4_quant: 27 VGPRs;  silu_and_mul_mxfp4_quant: 36 VGPRs;  no LDS, scratch 0, occupancy 8
// Nothing is allocated or synchronised and there is no workspace: every entry point is graph-capturable.
#include "quant_helpers.cuh"

#include <limits.h>

namespace va {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) int i32x8;

constexpr int MX_BLOCK = 32;     // values per e8m0 scale byte
constexpr int MX_KB = 128;       // K elements per MFMA = 64 bytes of codes and 4 scale bytes per row
constexpr int MX_WAVES = 8;

extern int g_moe_ks;   // moe_block_fp8.hip: tuning "moe_ks"

// ---------------------------------------------------------------------------------------------
// (a) the quantiser
// ---------------------------------------------------------------------------------------------
// e8m0 byte of a block from its amax (>= 0): exponent field - 2, one more from 1.75 on
__device__ __forceinline__ int mx_scale_byte(float amax) {
  const uint32_t bits = __float_as_uint(amax);
  const int e = (int)(bits >> 23) + ((bits & 0x7fffffu) >= 0x600000u ? 1 : 0) - 2;
  return min(max(e, 0), 254);
}

// e2m1 code (sign in bit 3) of x 2^sh, rounded to nearest-even onto the grid, saturating
__device__ __forceinline__ uint32_t mx_code(float x, int sh) {
  const float a = fminf(ldexpf(fabsf(x), sh), 6.0f);
  const float inv = a < 2.0f ? 2.0f : (a < 4.0f ? 1.0f : 0.5f);   // 1 / grid step
  const float r = __builtin_rintf(a * inv) * (a < 2.0f ? 0.5f : (a < 4.0f ? 1.0f : 2.0f));
  // from 1 on the code is exponent and first mantissa bit (1 -> 2, 1.5 -> 3, 2 -> 4 .. 6 -> 7); .5 -> 1
  const uint32_t mag = r >= 1.0f ? (__float_as_uint(r) >> 22) - 252u : (r > 0.0f ? 1u : 0u);
  return mag | ((__float_as_uint(x) >> 28) & 8u);
}

// The 8 values of a lane -> one dword of codes; the quad (4 lanes = one 32-block) shares the scale byte.
// Runs with all 64 lanes enabled.
__device__ __forceinline__ uint32_t mx_quant8(const float (&f)[8], int& byte) {
  float m = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(f[j]));
  m = fmaxf(m, dpp_move<0xB1>(m));    // quad_perm [1,0,3,2]
  m = fmaxf(m, dpp_move<0x4E>(m));    // quad_perm [2,3,0,1]
  byte = mx_scale_byte(m);
  uint32_t q = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) q |= mx_code(f[j], 127 - byte) << (4 * j);
  return q;
}

constexpr int MQ_WAVES = 4;

// FUSED: in is [rows, 2 d] contiguous and the value is silu(x) * y; else in is [rows, d] with row stride ld
template <typename T, bool FUSED>
__global__ __launch_bounds__(MQ_WAVES * 64) void mxfp4_quant_kernel(uint8_t* __restrict__ out_q,
                                                                    uint8_t* __restrict__ out_s,
                                                                    const T* __restrict__ in, int64_t num_rows, int d,
                                                                    int64_t ld) {
  const int lane = threadIdx.x & 63;
  const int cpr = d / 8;                            // lane chunks per row, a multiple of 4
  const int64_t total = num_rows * cpr;
  const int64_t wave = (int64_t)blockIdx.x * MQ_WAVES + (threadIdx.x >> 6);
  const int64_t step = (int64_t)gridDim.x * MQ_WAVES * 64;
  // the loop bounds are wave-uniform: the DPP runs with all 64 lanes enabled
  for (int64_t base = wave * 64; base < total; base += step) {
    const int64_t idx = base + lane;
    const bool ok = idx < total;
    const int64_t ii = ok ? idx : 0;                // idle lanes re-read chunk 0
    const int64_t row = ii / cpr;
    const int ch = (int)(ii - row * cpr);
    float f[8];
    if constexpr (FUSED) {
      const T* px = in + row * 2 * d + ch * 8;
      const Vec<T, 8> xv = *reinterpret_cast<const Vec<T, 8>*>(px);
      const Vec<T, 8> yv = *reinterpret_cast<const Vec<T, 8>*>(px + d);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = silu_mul<T>(xv.v[j], yv.v[j]);
    } else {
      load8<T>(in + row * ld + ch * 8, f);
    }
    int byte;
    const uint32_t q = mx_quant8(f, byte);
    if (ok) {
      *reinterpret_cast<uint32_t*>(out_q + row * (d / 2) + ch * 4) = q;
      if ((ch & 3) == 0) out_s[row * (d / MX_BLOCK) + (ch >> 2)] = (uint8_t)byte;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// (b) grouped GEMM
// ---------------------------------------------------------------------------------------------
// 16 x 16 x 128 over fp4 operands (cbsz 4, blgp 4): the codes sit in the low four registers, byte 0 of
// each scale register is the e8m0 scale of the lane's 32 values
__device__ __forceinline__ f32x4 mx_mfma(uint4 w, uint4 a, f32x4 c, uint32_t ws, uint32_t as) {
  const i32x8 wf = {(int)w.x, (int)w.y, (int)w.z, (int)w.w, 0, 0, 0, 0};
  const i32x8 af = {(int)a.x, (int)a.y, (int)a.z, (int)a.w, 0, 0, 0, 0};
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf, af, c, 4 /*fp4 e2m1*/, 4, 0, (int)ws, 0, (int)as);
}

template <typename out_t, int MT, int KS>
__global__ __launch_bounds__(MX_WAVES * 64) void moe_mxfp4_gemm_kernel(
    out_t* __restrict__ c, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
    const uint8_t* __restrict__ a_scales, const uint8_t* __restrict__ b_scales, const int* __restrict__ sorted_ids,
    const int* __restrict__ expert_ids, const int* __restrict__ num_post, const float* __restrict__ topk_w, int nvt,
    int top_k, int E, int N, int K, int max_padded, int nsg, int64_t lda, int64_t b_se, int64_t b_sn, int64_t ldc,
    int64_t as_sm, int64_t bs_se, int64_t bs_sn) {
  constexpr int NS = MX_WAVES / KS;   // strips per workgroup
  constexpr int BM = 16 * MT;
  constexpr int NA = MT == 1 ? 2 : 1;  // accumulators per m-tile
  __shared__ float red[MX_WAVES][MT][16][17];
  __shared__ int stok[BM];

  const int mb = blockIdx.x / nsg, sg = blockIdx.x - mb * nsg;
  // never past the caller's buffers, whatever the device-side count says
  const int padded = min(*num_post, max_padded);
  if (mb * BM >= padded) return;                  // workgroup-uniform
  const int e = expert_ids[mb];                   // workgroup-uniform

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c16 = lane & 15, g4 = lane >> 4;
  const int strip = wave / KS, kw = wave - strip * KS;
  const int n_wg = sg * NS * 16;                  // first column of the workgroup

  // flat slot of every sorted row; -1 = padding (never stored)
  if (tid < BM) {
    const int i = mb * BM + tid;
    const int t = i < padded ? sorted_ids[i] : nvt;
    stok[tid] = (unsigned)t < (unsigned)nvt ? t : -1;
  }

  if ((unsigned)e >= (unsigned)E) {
    // an expert of another rank (expert_map): zeros for the valid rows
    __syncthreads();
    for (int idx = tid; idx < BM * NS * 16; idx += MX_WAVES * 64) {
      const int r = idx / (NS * 16), n = n_wg + idx % (NS * 16);
      const int t = stok[r];
      if (t >= 0 && n < N) c[(int64_t)t * ldc + n] = from_f32<out_t>(0.f);
    }
    return;
  }

  const int n0 = n_wg + strip * 16;
  const int nkb = K / MX_KB;
  // rows past N and padding entries re-read a valid row: their outputs are never stored
  const int64_t wr = min(n0 + c16, N - 1);
  const uint8_t* wrow = b + (int64_t)e * b_se + wr * b_sn + 16 * g4;
  const uint8_t* wsrow = b_scales + (int64_t)e * bs_se + wr * bs_sn;
  const uint8_t* arow[MT];
  const uint8_t* asrow[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int i = mb * BM + t * 16 + c16;
    const int slot = i < padded ? sorted_ids[i] : nvt;
    const int m = (int)min((unsigned)slot, (unsigned)(nvt - 1)) / top_k;
    arow[t] = a + (int64_t)m * lda + 16 * g4;
    asrow[t] = a_scales + (int64_t)m * as_sm;
  }

  f32x4 acc[NA][MT];
#pragma unroll
  for (int i = 0; i < NA; ++i)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[i][t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  constexpr int UN = MT <= 2 ? 8 : 4;   // K blocks of loads in flight per wave
  const int ub = nkb >= 2 * KS ? 1 : 0;  // log2 of the round-robin unit: 2 blocks (a 128-byte line) or 1
  const int sh = 8 * g4;                // the lane's scale byte inside the block's dword
  for (int kb = kw << ub; kb < nkb; kb += UN * KS) {
    uint4 wv[UN], av[UN][MT];
    uint32_t ws[UN], as[UN][MT];
    int kbu[UN];                        // wave-uniform
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      kbu[u] = kb + ((u >> ub) << ub) * KS + (u & ub);
      if (kbu[u] < nkb) {
        wv[u] = *reinterpret_cast<const uint4*>(wrow + (int64_t)kbu[u] * (MX_KB / 2));
        ws[u] = *reinterpret_cast<const uint32_t*>(wsrow + 4 * kbu[u]);
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          av[u][t] = *reinterpret_cast<const uint4*>(arow[t] + (int64_t)kbu[u] * (MX_KB / 2));
          as[u][t] = *reinterpret_cast<const uint32_t*>(asrow[t] + 4 * kbu[u]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      if (kbu[u] < nkb) {
#pragma unroll
        for (int t = 0; t < MT; ++t)
          acc[u % NA][t] = mx_mfma(wv[u], av[u][t], acc[u % NA][t], ws[u] >> sh, as[u][t] >> sh);
      }
    }
  }
  // lane holds C^T[n = 4 g4 + r][m = 16 t + c16] of its strip
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = acc[0][t][r];
      if constexpr (NA == 2) v += acc[1][t][r];
      red[wave][t][c16][4 * g4 + r] = v;   // [m][n]
    }
  __syncthreads();
  // the KS partials in wave order, routed weight in fp32, one rounding; a row's NS * 16 columns are
  // adjacent threads
  for (int idx = tid; idx < BM * NS * 16; idx += MX_WAVES * 64) {
    const int nn = idx & 15, s = (idx >> 4) & (NS - 1), r = idx / (NS * 16);
    const int t = stok[r], n = n_wg + s * 16 + nn;
    if (t < 0 || n >= N) continue;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < KS; ++w) v += red[s * KS + w][r >> 4][r & 15][nn];
    if (topk_w) v *= topk_w[t];
    c[(int64_t)t * ldc + n] = from_f32<out_t>(v);
  }
}

}  // namespace va

using namespace va;

template <typename T>
static void launch_mxfp4_gemm(void* c, const void* a, const void* b, const void* as, const void* bs,
                              const int32_t* sorted_ids, const int32_t* expert_ids, const int32_t* num_post,
                              const float* topk_w, int nvt, int top_k, int bm, int E, int N, int K, int max_padded,
                              int64_t lda, int64_t b_se, int64_t b_sn, int64_t ldc, int64_t as_sm, int64_t bs_se,
                              int64_t bs_sn, hipStream_t st) {
  // Waves per strip ("moe_ks").  The fp8 kernel's measured rule was: 8 for a long row (K >= 2048 bytes) under a
  // narrow output (N <= 1024, where four strips per workgroup leave too few workgroups for 256 CUs), else 2.  A
  // wave's share of a row is what matters, and a row here is K / 2 bytes, so the same rule in bytes puts the
  // threshold at K >= 4096: 32 K blocks, four per wave with KS 8.  Measured (tools/bench_moe.py --mxfp4,
  // profiles/moe_mxfp4.txt; E 256, top-k 8, block_size_m 16), KS 8 / KS 2 in us at 1 / 16 / 64 / 256 tokens:
  //   N 4096 K 7168: 36.1 / 33.8,  432 / 395, 1045 / 962, 1312 / 1338    N 7168 K 2048: 28.1 / 23.7, 336 / 211, 805 / 505, 1040 / 680
  //   N  512 K 7168:  7.4 / 17.7, 56.0 / 53.3, 137 / 137,  171 / 184     N 7168 K  256: 12.6 /  6.4, 144 / 46.4, 333 / 107, 443 / 157
  // The rule picks the faster value everywhere but N 512 at 16 tokens (5 %) and N 4096 at 256 tokens (2 %).  The N
  // threshold lies between the measured 512 and 4096, the K threshold between 2048 and 7168: neither is measured.
  const int nkb = K / MX_KB;
  const int ks = g_moe_ks == 8 || g_moe_ks == 2 ? g_moe_ks : (nkb >= 32 && N <= 1024 ? 8 : 2);
  const int nsg = ceil_div(N, 16 * (MX_WAVES / ks));
  const int mblocks = ceil_div(max_padded, bm);
#define MG(MT, KS)                                                                                              \
  hipLaunchKernelGGL((moe_mxfp4_gemm_kernel<T, MT, KS>), dim3((unsigned)(mblocks * nsg)), dim3(MX_WAVES * 64),  \
                     0, st, (T*)c, (const uint8_t*)a, (const uint8_t*)b, (const uint8_t*)as, (const uint8_t*)bs, \
                     sorted_ids, expert_ids, num_post, topk_w, nvt, top_k, E, N, K, max_padded, nsg, lda, b_se, \
                     b_sn, ldc, as_sm, bs_se, bs_sn)
  if (bm == 16) { if (ks == 8) MG(1, 8); else MG(1, 2); }
  else { if (ks == 8) MG(4, 8); else MG(4, 2); }
#undef MG
}

extern "C" int vllm_amd_moe_mxfp4_gemm(void* c, const void* a, const void* b, const void* a_scales,
                                       const void* b_scales, const int32_t* sorted_token_ids,
                                       const int32_t* expert_ids, const int32_t* num_tokens_post_padded,
                                       const float* topk_weights, int num_valid_tokens, int top_k,
                                       int mul_routed_weight, int block_size_m, int max_num_tokens_padded,
                                       int num_experts, int N, int K, int64_t lda, int64_t b_stride_e,
                                       int64_t b_stride_n, int64_t ldc, int64_t as_stride_m, int64_t bs_stride_e,
                                       int64_t bs_stride_n, int out_dtype, void* stream) {
  const char* op = "moe_mxfp4_gemm";
  VA_REQUIRE(num_valid_tokens >= 0 && N >= 0 && K >= 0 && num_experts >= 0, VLLM_AMD_EINVAL, "%s: negative dimension", op);
  VA_REQUIRE(block_size_m == 16 || block_size_m == 64, VLLM_AMD_EUNSUPPORTED,
             "%s: block_size_m = %d must be 16 or 64", op, block_size_m);
  VA_REQUIRE(out_dtype == VLLM_AMD_BF16 || out_dtype == VLLM_AMD_F16, VLLM_AMD_EUNSUPPORTED,
             "%s: out dtype must be bfloat16 or float16", op);
  VA_REQUIRE(K > 0 && K % MX_KB == 0, VLLM_AMD_EUNSUPPORTED,
             "%s: K = %d must be a positive multiple of 128 (one scaled MFMA: four 32-wide MX blocks)", op, K);
  VA_REQUIRE(top_k >= 1 && num_valid_tokens % top_k == 0, VLLM_AMD_EINVAL,
             "%s: num_valid_tokens %d is not a multiple of top_k %d", op, num_valid_tokens, top_k);
  if (num_valid_tokens == 0 || N == 0 || num_experts == 0) return VLLM_AMD_OK;
  VA_REQUIRE(c && a && b && a_scales && b_scales && sorted_token_ids && expert_ids && num_tokens_post_padded,
             VLLM_AMD_EINVAL, "%s: null pointer", op);
  VA_REQUIRE(!mul_routed_weight || topk_weights, VLLM_AMD_EINVAL, "%s: mul_routed_weight without topk_weights", op);
  VA_REQUIRE(lda % 16 == 0 && b_stride_n % 16 == 0 && b_stride_e % 16 == 0 && lda >= K / 2 && b_stride_n >= K / 2 &&
                 (((uintptr_t)a) & 15) == 0 && (((uintptr_t)b) & 15) == 0,
             VLLM_AMD_EUNSUPPORTED,
             "%s: lda, the weight strides (>= K / 2 bytes) and operand pointers must be multiples of 16", op);
  VA_REQUIRE(as_stride_m % 4 == 0 && bs_stride_n % 4 == 0 && bs_stride_e % 4 == 0 && as_stride_m >= K / MX_BLOCK &&
                 bs_stride_n >= K / MX_BLOCK && (((uintptr_t)a_scales) & 3) == 0 && (((uintptr_t)b_scales) & 3) == 0,
             VLLM_AMD_EUNSUPPORTED,
             "%s: the scale strides (>= K / 32 bytes) and scale pointers must be multiples of 4", op);
  VA_REQUIRE(ldc >= N, VLLM_AMD_EINVAL, "%s: ldc < N", op);
  VA_REQUIRE(max_num_tokens_padded >= num_valid_tokens, VLLM_AMD_EINVAL,
             "%s: max_num_tokens_padded %d < num_valid_tokens %d", op, max_num_tokens_padded, num_valid_tokens);
  const int64_t max_padded = max_num_tokens_padded;
  const int64_t wgs = ((max_padded + block_size_m - 1) / block_size_m) * (int64_t)ceil_div(N, 16);
  VA_REQUIRE(wgs < INT_MAX, VLLM_AMD_EUNSUPPORTED, "%s: too many workgroups", op);
  hipStream_t st = (hipStream_t)stream;
  const float* tw = mul_routed_weight ? topk_weights : nullptr;
  if (out_dtype == VLLM_AMD_BF16)
    launch_mxfp4_gemm<bf16_t>(c, a, b, a_scales, b_scales, sorted_token_ids, expert_ids, num_tokens_post_padded, tw,
                              num_valid_tokens, top_k, block_size_m, num_experts, N, K, (int)max_padded, lda,
                              b_stride_e, b_stride_n, ldc, as_stride_m, bs_stride_e, bs_stride_n, st);
  else
    launch_mxfp4_gemm<f16_t>(c, a, b, a_scales, b_scales, sorted_token_ids, expert_ids, num_tokens_post_padded, tw,
                             num_valid_tokens, top_k, block_size_m, num_experts, N, K, (int)max_padded, lda,
                             b_stride_e, b_stride_n, ldc, as_stride_m, bs_stride_e, bs_stride_n, st);
  VA_LAUNCH_CHECK("moe_mxfp4_gemm launch");
  return VLLM_AMD_OK;
}

template <bool FUSED>
static int launch_mxfp4_quant(const char* op, void* out_q, void* out_s, const void* input, int64_t num_rows, int d,
                              int64_t ld, int dtype, void* stream) {
  VA_REQUIRE(num_rows >= 0 && d >= 0, VLLM_AMD_EINVAL, "%s: bad shape", op);
  VA_REQUIRE(d % MX_BLOCK == 0, VLLM_AMD_EUNSUPPORTED, "%s: row length %d is not a multiple of the 32-wide MX block",
             op, d);
  VA_REQUIRE(dtype == VLLM_AMD_F16 || dtype == VLLM_AMD_BF16, VLLM_AMD_EUNSUPPORTED,
             "%s: input must be float16 or bfloat16", op);
  if (num_rows == 0 || d == 0) return VLLM_AMD_OK;
  VA_REQUIRE(out_q && out_s && input, VLLM_AMD_EINVAL, "%s: null pointer", op);
  VA_REQUIRE(ld >= d && ld % 8 == 0 && (((uintptr_t)input) & 15) == 0 && (((uintptr_t)out_q) & 3) == 0,
             VLLM_AMD_EUNSUPPORTED,
             "%s: the row stride (>= row length) must be a multiple of 8 elements, input 16-byte and output 4-byte "
             "aligned", op);
  const int64_t chunks = num_rows * (d / 8);
  int64_t grid = (chunks + MQ_WAVES * 64 - 1) / (MQ_WAVES * 64);
  if (grid > 256 * 8) grid = 256 * 8;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == VLLM_AMD_F16)
    hipLaunchKernelGGL((mxfp4_quant_kernel<f16_t, FUSED>), dim3((unsigned)grid), dim3(MQ_WAVES * 64), 0, st,
                       (uint8_t*)out_q, (uint8_t*)out_s, (const f16_t*)input, num_rows, d, ld);
  else
    hipLaunchKernelGGL((mxfp4_quant_kernel<bf16_t, FUSED>), dim3((unsigned)grid), dim3(MQ_WAVES * 64), 0, st,
                       (uint8_t*)out_q, (uint8_t*)out_s, (const bf16_t*)input, num_rows, d, ld);
  VA_LAUNCH_CHECK(op);
  return VLLM_AMD_OK;
}

extern "C" int vllm_amd_mxfp4_quant(void* out_q, void* out_s, const void* input, int64_t num_rows, int K,
                                    int64_t row_stride, int dtype, void* stream) {
  return launch_mxfp4_quant<false>("mxfp4_quant", out_q, out_s, input, num_rows, K, row_stride, dtype, stream);
}

extern "C" int vllm_amd_silu_and_mul_mxfp4_quant(void* out_q, void* out_s, const void* input, int64_t num_rows,
                                                 int d, int dtype, void* stream) {
  return launch_mxfp4_quant<true>("silu_and_mul_mxfp4_quant", out_q, out_s, input, num_rows, d, 2 * (int64_t)d,
                                  dtype, stream);
}
