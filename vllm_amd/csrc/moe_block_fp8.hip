// Fused MoE experts over block-scaled fp8 (OCP e4m3fn) weights for gfx950: the four kernels behind
// fused_experts(..., use_fp8_w8a8=True, block_shape=[128, 128])
// (vllm/model_executor/layers/fused_moe/fused_moe.py:1349-1563 of the reference):
//
//   moe_align_block_size        topk_ids -> expert-sorted, block-padded token list
//   moe_blockwise_gemm          grouped GEMM, 128 x 128 weight scales, 1 x 128 activation scales
//   silu_and_mul_group_quant    activation + 1 x 128 quantiser between the two GEMMs
//   moe_sum                     reduction over the top-k axis
//
// (a) Grouped GEMM.  Semantics of the reference's Triton fused_moe_kernel (fused_moe.py:268-475): entry
//     i of sorted_token_ids names flat (token, k) slot t; A row t / top_k meets the weights of
//     expert_ids[i / block_size_m] and lands in C row t.  An entry >= num_valid_tokens is padding: it
//     reads a clamped row and is never stored.  A block of expert -1 stores zeros, blocks past
//     *num_tokens_post_padded exit; the real count is read on the device, the grid is the host-side
//     upper bound (the length of sorted_token_ids, which with an expert_map was aligned for the global
//     expert count; the local count only decides which expert ids store zeros), so nothing is synchronised.
//
//     It is a weight-streaming kernel (decode: every expert sees a handful of rows, the experts' weight
//     bytes are the traffic).  A workgroup of 8 waves serves ONE m-block (16 or 64 sorted rows = MT = 1
//     or 4 MFMA row tiles) of ONE expert -- the expert id is read once and is workgroup-uniform -- and
//     8 / KS strips of 16 output columns, KS waves per strip taking the strip's K blocks round-robin:
//       KS = 2: four strips per workgroup; every wave has weight bytes to stream down to K = 256 =
//               2 blocks (where the KS = 8 split would idle six waves), and measured faster at long K
//               too wherever N gives enough workgroups (see launch_moe_gemm);
//       KS = 8: one strip per workgroup, the split of scaled_mm_block_stream_kernel: narrow outputs
//               with a long K (N 512, K 7168), where it gives four times the workgroups.
//     Per K block one v_mfma_scale_f32_16x16x128_f8f6f4 with a zero C operand per m-tile, computed
//     transposed (A operand = weight rows), folded with acc = fma(partial, As * Bs, acc).  Fragments go
//     from global memory straight to VGPRs in that kernel's K permutation (lane group g takes bytes
//     64 j + 16 g), UN = 4 (MT 1) or 2 (MT 4) K blocks of loads in flight per wave.  The weight-scale
//     column is wave-uniform (16 | 128).  The KS partial sums of a strip meet in LDS; then routed
//     weight (fp32, before the single rounding), cast, and the scattered row store: the 16 (KS 8) or
//     64 (KS 2) columns of a row are contiguous.
//     Launch order: blockIdx.x = m_block * strip_groups + strip_group, so the workgroups of an expert
//     are adjacent, and the next m-block of a busy expert follows its first while the weights are in L2.
//
// (a') Grouped tile kernel, block_size_m = 128 (prefill: an expert sees a hundred rows or more, and
//     the streaming form would read its weights again for every 64 of them).  The same contract; the
//     data movement of scaled_mm_block_tile_kernel<out_t, 128> (scaled_mm_block.hip) over a gathered A
//     operand.  A workgroup of 4 waves owns 128 sorted rows of ONE expert x 128 output columns = one
//     weight-scale column, so Bs[e, n0 / 128, kb] is a scalar load; every wave a 64 x 64 sub-tile =
//     4 x 4 MFMA tiles, zero C operand, folded with fma(partial, As * Bs, acc) into ONE sequential fp32
//     accumulator (the streaming form adds KS partial sums: results differ in the last bits).
//     Staging is global_load_lds, 16 B per lane, into the XOR-swizzled [rows][128 B] image, a ring of 4
//     stages, one barrier per K block.  The source address of an LDS-DMA is per lane, so the gather
//     is free: a staging lane reads its rows' slots from sorted_token_ids once, before the loop,
//     clamps them, and keeps a + (slot / top_k) * lda; the weight rows come from b + e * b_stride_e.
//     The 128 activation scales of a K block travel with the stage (one 4-byte LDS-DMA per lane,
//     gathered by the same row index through as_stride_m / as_stride_k), so the loop's only
//     vector-memory instructions are the 9 LDS-DMAs per stage that every wave issues, and the one
//     hand-counted s_waitcnt vmcnt((4 - 2) * 9) in front of the barrier is provable (checked in the
//     ISA: the slot loads are all waited for in front of the first LDS-DMA).
//     Epilogue: routed weight of the row in fp32, one rounding, the 128 x 128 image in LDS over the
//     stages, then whole rows scattered to C row t in 16-byte pieces (scalar where c, ldc or a ragged
//     N do not allow); padding rows are skipped, an absent expert stores zeros through the same loop.
//     Grid: ceil(max_num_tokens_padded / 128) x ceil(N / 128) workgroups, a host-side bound.  The
//     USED count comes from *num_tokens_post_padded; workgroups past it exit before any barrier, the
//     others are renumbered so that each of the 8 XCDs (hardware workgroup i runs on XCD i % 8) gets
//     one contiguous run of (m-block, n-tile) pairs, n-tile fastest: the n-tiles of an m-block share
//     its gathered rows in that XCD's L2, and the next m-block of a busy expert follows while its
//     weight panels may still be there.  The run is cut from the used count: cut from the grid, the
//     last XCDs would hold nothing but exiting workgroups.  Effect on L2 hits: not measured.
//     The MFMAs of 16-row tiles that hold only padding are NOT skipped (not built, not measured).
//
// (b) moe_align_block_size: one workgroup of 1024 threads; LDS histogram over the experts, block-wide
//     exclusive scan of the padded counts, expert_ids by binary search over the segment starts, then
//     the scatter through LDS cursors.  Ids outside [0, E) are skipped (the reference would index out
//     of bounds).  The order inside a segment is unspecified.  expert_ids past the last used block are
//     set to 0, so that indexing an expert_map with the whole tensor is defined.
//
// (c) silu_and_mul_group_quant: the group quantiser's work split (group_quant.hip: 16 lanes x 8
//     elements per 128-group, DPP maximum, Markstein quotient) on v = T(T(silu(x)) * y) computed in
//     registers: one read of [rows, 2 I], no 16-bit intermediate tensor.
//
// (d) moe_sum: out[t, :] = sum_k in[t, k, :], accumulated in fp32 in k order and rounded once, 16-byte
//     accesses where alignment allows.  DEVIATION: the reference (csrc/moe/moe_align_sum_kernels.cu)
//     accumulates top-k 2, 3 and 4 in the 16-bit type (one rounding per addition); this kernel is at
//     least as accurate, and not bit-identical to it for top-k >= 3.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage, bf16 out):
//   gemm MT 1, KS 8 / 2: 104 / 104 VGPRs, 0 AGPRs, scratch 0, LDS  8768 B, occupancy 4 waves / SIMD
//   gemm MT 4, KS 8 / 2: 150 / 148 VGPRs, 0 AGPRs, scratch 0, LDS 35072 B, occupancy 3 waves / SIMD
//   gemm tile 128: 166 VGPRs + 20 AGPRs, scratch 0, LDS 133632 B, 1 workgroup (4 waves) / CU = 1 wave / SIMD
//   align: 26 VGPRs, LDS 8260 B;  silu_and_mul_group_quant: 45 VGPRs, no LDS;  moe_sum: 30 VGPRs, no LDS;
//   all scratch 0, occupancy 8
// Nothing is allocated or synchronised and there is no workspace: every entry point is graph-capturable.
#include "quant_helpers.cuh"

#include <limits.h>

namespace va {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) int i32x8;

constexpr int MOE_QB = 128;      // scale block edge = K bytes per MFMA
constexpr int MOE_WAVES = 8;

int g_moe_ks = 0;   // tuning "moe_ks": 0 = by N and K, 8 / 2 = that many waves per 16-column strip

__device__ __forceinline__ f32x4 moe_block_mfma(i32x8 w, i32x8 a) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, a, (f32x4){0.f, 0.f, 0.f, 0.f}, 0 /*fp8 e4m3*/, 0, 0,
                                                          0x7f7f7f7f, 0, 0x7f7f7f7f);
}
__device__ __forceinline__ i32x8 moe_frag8(uint4 lo, uint4 hi) {
  return (i32x8){(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
}

// ---------------------------------------------------------------------------------------------
// (a) grouped GEMM
// ---------------------------------------------------------------------------------------------
template <typename out_t, int MT, int KS>
__global__ __launch_bounds__(MOE_WAVES * 64) void moe_block_gemm_kernel(
    out_t* __restrict__ c, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
    const float* __restrict__ a_scales, const float* __restrict__ b_scales, const int* __restrict__ sorted_ids,
    const int* __restrict__ expert_ids, const int* __restrict__ num_post, const float* __restrict__ topk_w, int nvt,
    int top_k, int E, int N, int K, int max_padded, int nsg, int64_t lda, int64_t b_se, int64_t b_sn, int64_t ldc,
    int64_t as_sm, int64_t as_sk, int64_t bs_se, int64_t bs_sn, int64_t bs_sk) {
  constexpr int NS = MOE_WAVES / KS;   // strips per workgroup
  constexpr int BM = 16 * MT;
  __shared__ float red[MOE_WAVES][MT][16][17];
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
    // an expert of another rank (expert_map): zeros for the valid rows (fused_moe.py:370-377)
    __syncthreads();
    for (int idx = tid; idx < BM * NS * 16; idx += MOE_WAVES * 64) {
      const int r = idx / (NS * 16), n = n_wg + idx % (NS * 16);
      const int t = stok[r];
      if (t >= 0 && n < N) c[(int64_t)t * ldc + n] = from_f32<out_t>(0.f);
    }
    return;
  }

  const int n0 = n_wg + strip * 16;
  const int nkb = K / MOE_QB;
  // rows past N and padding entries re-read a valid row: their outputs are never stored
  const uint8_t* wrow = b + (int64_t)e * b_se + (int64_t)min(n0 + c16, N - 1) * b_sn + 16 * g4;
  const float* bs_ptr = b_scales + (int64_t)e * bs_se + (int64_t)(min(n0, N - 1) / MOE_QB) * bs_sn;
  const uint8_t* arow[MT];
  const float* as_ptr[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int i = mb * BM + t * 16 + c16;
    const int slot = i < padded ? sorted_ids[i] : nvt;
    const int m = (int)min((unsigned)slot, (unsigned)(nvt - 1)) / top_k;
    arow[t] = a + (int64_t)m * lda + 16 * g4;
    as_ptr[t] = a_scales + (int64_t)m * as_sm;
  }

  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  constexpr int UN = MT <= 2 ? 4 : 2;   // K blocks of loads in flight per wave
  for (int kb = kw; kb < nkb; kb += UN * KS) {
    uint4 wv[UN][2], av[UN][MT][2];
    float as[UN][MT], bs[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int kbu = kb + u * KS;               // wave-uniform
      if (kbu < nkb) {
        const int64_t k = (int64_t)kbu * MOE_QB;   // + 16 g4 is in the row pointers
#pragma unroll
        for (int j = 0; j < 2; ++j) wv[u][j] = *reinterpret_cast<const uint4*>(wrow + k + 64 * j);
#pragma unroll
        for (int t = 0; t < MT; ++t) {
#pragma unroll
          for (int j = 0; j < 2; ++j) av[u][t][j] = *reinterpret_cast<const uint4*>(arow[t] + k + 64 * j);
          as[u][t] = as_ptr[t][(int64_t)kbu * as_sk];
        }
        bs[u] = bs_ptr[(int64_t)kbu * bs_sk];
      }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      if (kb + u * KS < nkb) {
        const i32x8 wf = moe_frag8(wv[u][0], wv[u][1]);
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          const f32x4 p = moe_block_mfma(wf, moe_frag8(av[u][t][0], av[u][t][1]));
          const float s = as[u][t] * bs[u];
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[t][r] = fmaf(p[r], s, acc[t][r]);
        }
      }
    }
  }
  // lane holds C^T[n = 4 g4 + r][m = 16 t + c16] of its strip
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][t][c16][4 * g4 + r] = acc[t][r];   // [m][n]
  __syncthreads();
  // the KS partials in wave order, routed weight in fp32, one rounding; a row's NS * 16 columns are
  // adjacent threads
  for (int idx = tid; idx < BM * NS * 16; idx += MOE_WAVES * 64) {
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

// ---------------------------------------------------------------------------------------------
// (a') grouped tile kernel, block_size_m 128
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int moe_qswz(int row) {
  return ((row >> 1) & 1) | (((row >> 2) & 1) << 2);
}
// LDS reads of the K loop as inline asm: a C++ LDS load is ordered by hipcc behind ALL outstanding
// LDS-DMA (s_waitcnt vmcnt(0)), which would serialise the ring with the math
typedef __attribute__((ext_vector_type(4))) int i32x4;
template <int OFF>
__device__ __forceinline__ i32x4 moe_lds_read16(uint32_t addr) {
  i32x4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}
template <int OFF>
__device__ __forceinline__ float moe_lds_read4(uint32_t addr) {
  float v;
  asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}

constexpr int MOE_TILE_BM = 128;

template <typename out_t>
__global__ __launch_bounds__(MOE_TILE_BM * 2) void moe_block_gemm_tile_kernel(
    out_t* __restrict__ c, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
    const float* __restrict__ a_scales, const float* __restrict__ b_scales, const int* __restrict__ sorted_ids,
    const int* __restrict__ expert_ids, const int* __restrict__ num_post, const float* __restrict__ topk_w, int nvt,
    int top_k, int E, int N, int K, int max_padded, int tiles_n, int64_t lda, int64_t b_se, int64_t b_sn, int64_t ldc,
    int64_t as_sm, int64_t as_sk, int64_t bs_se, int64_t bs_sn, int64_t bs_sk, int vec_store) {
  constexpr int BM = MOE_TILE_BM, QB = MOE_QB;
  constexpr int NW = BM / 32;                        // 4 waves: 2 x 2, each 64 x 64
  constexpr int A_BYTES = BM * QB, W_BYTES = QB * QB, STAGE = A_BYTES + W_BYTES;
  constexpr int RPR = 8 * NW;                        // rows staged per glds round
  constexpr int A_ROUNDS = BM / RPR, W_ROUNDS = QB / RPR;
  constexpr int OROW = QB + 8;                       // output image: row stride in elements (272 B)
  constexpr int NST = 4;                             // ring stages: NST - 1 K blocks in flight
  constexpr int STRIP = BM * 4;                      // the BM activation scales of a K block
  constexpr int PER = A_ROUNDS + W_ROUNDS + 1;       // LDS-DMA instructions per lane and stage
  static_assert(BM * OROW * (int)sizeof(out_t) <= NST * STAGE, "the output image overlays the stages");
  static_assert(NST * (STAGE + STRIP) + BM * 4 <= 160 * 1024 && (NST - 2) * PER <= 63, "LDS size, vmcnt is 6 bits");
  __shared__ __attribute__((aligned(16))) uint8_t lds[NST * (STAGE + STRIP)];
  __shared__ int stok[BM];

  // The grid is the host-side bound; the blocks in use are counted here.  Hardware workgroup i runs on
  // XCD i % 8: give every XCD a contiguous run of the USED (m-block, n-tile) pairs, n fastest, so that
  // the n-tiles of an m-block (which share its 128 gathered rows) and the next m-block of the same
  // expert (which shares its weight panels) meet in one L2.  The run is cut from the used count, not
  // from the grid, or the last XCDs would hold only blocks that exit.
  const int padded = min(*num_post, max_padded);     // never past the caller's buffers
  const int used = (padded + BM - 1) / BM * tiles_n;
  int wg = blockIdx.x;
  if (wg >= used) return;                            // workgroup-uniform, before any barrier
  {
    const int q = used / 8, r = used % 8, xcd = wg % 8, idx = wg / 8;
    wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const int mb = wg / tiles_n, tn = wg - mb * tiles_n;
  const int m0 = mb * BM, n0 = tn * QB;
  const int e = __builtin_amdgcn_readfirstlane(expert_ids[mb]);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c16 = lane & 15, g4 = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;

  // flat slot of a sorted row, nvt or more = padding
  auto slot_of = [&](int row) { return m0 + row < padded ? sorted_ids[m0 + row] : nvt; };
  if (tid < BM) {
    const int t = slot_of(tid);
    stok[tid] = (unsigned)t < (unsigned)nvt ? t : -1;   // -1: never stored
  }

  // whole rows out of the image in LDS (or zeros): thread -> 16-byte piece tid & 15 of rows tid >> 4, + 16, ...
  out_t* ot = reinterpret_cast<out_t*>(lds);
  auto store_rows = [&](bool zero) {
    const int chunk = tid & 15;
    const int n = n0 + chunk * 8;
    if (n >= N) return;
    for (int row = tid >> 4; row < BM; row += NW * 4) {
      const int t = stok[row];
      if (t < 0) continue;
      uint4 v = {0u, 0u, 0u, 0u};                    // sixteen zero bytes are eight zeros of either type
      if (!zero) v = *reinterpret_cast<const uint4*>(ot + row * OROW + chunk * 8);
      out_t* op = c + (int64_t)t * ldc + n;
      if (vec_store && n + 8 <= N) {
        *reinterpret_cast<uint4*>(op) = v;
      } else {
        const out_t* ev = reinterpret_cast<const out_t*>(&v);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (n + j < N) op[j] = ev[j];
      }
    }
  };

  if ((unsigned)e >= (unsigned)E) {
    // an expert of another rank (expert_map): zeros for the valid rows
    __syncthreads();
    store_rows(true);
    return;
  }

  // staging: in round r wave w fills rows [RPR r + 8 w, +8); lane -> (row = lane >> 3, slot = lane & 7)
  // loads logical chunk slot ^ f(row), so the lane-linear LDS image is the swizzled tile.  The A source
  // is per lane, so the gather costs nothing: the lane reads its row's slot once, here.  Padding
  // entries and weight rows past N re-read a valid row: their outputs are never stored.
  const int srow = lane >> 3, sslot = lane & 7;
  const uint8_t* a_src[A_ROUNDS];
  const uint8_t* w_src[W_ROUNDS];
#pragma unroll
  for (int r = 0; r < A_ROUNDS; ++r) {
    const int row = RPR * r + 8 * wave + srow;
    const int m = (int)min((unsigned)slot_of(row), (unsigned)(nvt - 1)) / top_k;
    a_src[r] = a + (int64_t)m * lda + ((sslot ^ moe_qswz(row)) << 4);
  }
#pragma unroll
  for (int r = 0; r < W_ROUNDS; ++r) {
    const int row = RPR * r + 8 * wave + srow;
    const int n = min(n0 + row, N - 1);
    w_src[r] = b + (int64_t)e * b_se + (int64_t)n * b_sn + ((sslot ^ moe_qswz(row)) << 4);
  }
  // the activation scales of a K block travel with its tile: every wave gathers 64 of the 128 values
  // As[row of slot, kb] into the stage's strip with one 4-byte LDS-DMA (waves 2 and 3 repeat the rows
  // of waves 0 and 1: the same values to the same place, so every wave counts PER loads)
  const int strip_row = (wave & 1) * 64;
  const float* as_src =
      a_scales + (int64_t)((int)min((unsigned)slot_of(strip_row + lane), (unsigned)(nvt - 1)) / top_k) * as_sm;
  auto stage_load = [&](int stage, int kb) {
    uint8_t* base = lds + stage * STAGE + 8 * wave * QB;
    const int64_t k0 = (int64_t)kb * QB;
#pragma unroll
    for (int r = 0; r < A_ROUNDS; ++r)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a_src[r] + k0),
                                       (__attribute__((address_space(3))) void*)(base + RPR * r * QB), 16, 0, 0);
#pragma unroll
    for (int r = 0; r < W_ROUNDS; ++r)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(w_src[r] + k0),
                                       (__attribute__((address_space(3))) void*)(base + A_BYTES + RPR * r * QB), 16, 0,
                                       0);
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)(as_src + (int64_t)kb * as_sk),
        (__attribute__((address_space(3))) void*)(lds + NST * STAGE + stage * STRIP + strip_row * 4), 4, 0, 0);
  };
  const float* bs_ptr = b_scales + (int64_t)e * bs_se + (int64_t)tn * bs_sn;   // workgroup-uniform

  f32x4 acc[4][4];   // [nt][mt]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // fragment read addresses: the swizzle depends on c16 only, so tile t is an immediate offset
  // t * 16 * 128 from one per-lane base per 16-byte half (j) and operand; likewise the lane's four
  // activation scales (row c16 of each of its m-tiles) in the strip
  const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)lds;
  uint32_t w_addr[2], a_addr[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int ch = ((2 * g4 + j) ^ moe_qswz(c16)) << 4;
    w_addr[j] = lds_base + A_BYTES + (wn * 64 + c16) * QB + ch;
    a_addr[j] = lds_base + (wm * 64 + c16) * QB + ch;
  }
  const uint32_t s_addr = lds_base + NST * STAGE + (wm * 64 + c16) * 4;

  // Ring of NST stages, NST - 1 K blocks in flight.  Per block: wait for the own LDS-DMA of block kb
  // (everything but the NST - 2 younger stages; near the end fewer are in flight, so drain) ->
  // s_barrier (everybody's has landed, and everybody is past its reads of the stage refilled next) ->
  // request all fragments and the four scales of the block -> issue the DMA of block kb + NST - 1 ->
  // lgkmcnt(0) -> 16 MFMAs with a zero C operand, each folded into the accumulators by 4 FMAs.
  // The slot reads above are ordinary vector loads: they stay in front of the first LDS-DMA, so that
  // the wait below counts LDS-DMAs only.
  const int nk = K / QB;
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int s = 0; s < NST - 1; ++s)
    if (s < nk) stage_load(s, s);
  int cur = 0, nxt = NST - 1;   // stage of block kb / of block kb + NST - 1
  for (int kb = 0; kb < nk; ++kb) {
    if (kb + NST - 1 <= nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST - 2) * PER) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    const uint32_t so = cur * STAGE;
    const uint32_t wa0 = w_addr[0] + so, wa1 = w_addr[1] + so, aa0 = a_addr[0] + so, aa1 = a_addr[1] + so;
    const uint32_t sa = s_addr + cur * STRIP;
    i32x4 wl[4], wh[4], al[4], ah[4];
    float as[4];
    static_for<4>([&](auto tc) {
      constexpr int t = decltype(tc)::value;
      wl[t] = moe_lds_read16<t * 16 * QB>(wa0);
      wh[t] = moe_lds_read16<t * 16 * QB>(wa1);
      al[t] = moe_lds_read16<t * 16 * QB>(aa0);
      ah[t] = moe_lds_read16<t * 16 * QB>(aa1);
      as[t] = moe_lds_read4<t * 64>(sa);
    });
    if (kb + NST - 1 < nk) stage_load(nxt, kb + NST - 1);
    cur = cur + 1 == NST ? 0 : cur + 1;
    nxt = nxt + 1 == NST ? 0 : nxt + 1;
    const float bs = bs_ptr[(int64_t)kb * bs_sk];
    // the fragments pass through the wait as in/out operands, so their consumers stay behind it
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(wl[0]), "+v"(wl[1]), "+v"(wl[2]), "+v"(wl[3]), "+v"(wh[0]), "+v"(wh[1]), "+v"(wh[2]),
                   "+v"(wh[3]), "+v"(al[0]), "+v"(al[1]), "+v"(al[2]), "+v"(al[3]), "+v"(ah[0]), "+v"(ah[1]),
                   "+v"(ah[2]), "+v"(ah[3]), "+v"(as[0]), "+v"(as[1]), "+v"(as[2]), "+v"(as[3]));
    __builtin_amdgcn_sched_barrier(0);

    i32x8 wf[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) wf[t] = __builtin_shufflevector(wl[t], wh[t], 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const float s = as[mt] * bs;
      const i32x8 af = __builtin_shufflevector(al[mt], ah[mt], 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const f32x4 p = moe_block_mfma(wf[nt], af);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[nt][mt][r] = fmaf(p[r], s, acc[nt][mt][r]);
      }
    }
  }

  // ---- epilogue: lane holds C^T[n = 16 nt + 4 g4 + r][m = 16 mt + c16]; routed weight of the row in
  // fp32, one rounding, through LDS (overlaying the stages), whole rows out to C row stok[row]
  __syncthreads();   // everybody is past its fragment reads
  float rw[4] = {1.f, 1.f, 1.f, 1.f};
  if (topk_w) {
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int t = stok[wm * 64 + mt * 16 + c16];
      if (t >= 0) rw[mt] = topk_w[t];
    }
  }
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int nl = wn * 64 + nt * 16 + 4 * g4;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int ml = wm * 64 + mt * 16 + c16;
      struct alignas(8) V4 { out_t e[4]; } pk;
#pragma unroll
      for (int r = 0; r < 4; ++r) pk.e[r] = from_f32<out_t>(acc[nt][mt][r] * rw[mt]);   // x 1.0f is exact
      *reinterpret_cast<V4*>(ot + ml * OROW + nl) = pk;
    }
  }
  __syncthreads();
  store_rows(false);
}

// ---------------------------------------------------------------------------------------------
// (b) moe_align_block_size
// ---------------------------------------------------------------------------------------------
constexpr int ALIGN_THREADS = 1024;   // = the largest expert count

__global__ __launch_bounds__(ALIGN_THREADS) void moe_align_kernel(
    const int* __restrict__ topk_ids, int* __restrict__ sorted_ids, int* __restrict__ expert_ids,
    int* __restrict__ num_post, int numel, int E, int bs, int max_padded, int max_blocks) {
  __shared__ int hist[ALIGN_THREADS];     // counts, then segment starts
  __shared__ int cursor[ALIGN_THREADS];
  __shared__ int wsum[ALIGN_THREADS / 64];
  __shared__ int total_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  hist[tid] = 0;
  __syncthreads();
  for (int i = tid; i < numel; i += ALIGN_THREADS) {
    const int e = topk_ids[i];
    if ((unsigned)e < (unsigned)E) atomicAdd(&hist[e], 1);
  }
  __syncthreads();

  // exclusive scan of the padded counts: inclusive inside the wave, then the 16 wave totals
  const int cnt = tid < E ? hist[tid] : 0;
  const int pad = (cnt + bs - 1) / bs * bs;
  int x = pad;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63) wsum[wave] = x;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int w = 0; w < ALIGN_THREADS / 64; ++w) {
      const int v = wsum[w];
      wsum[w] = run;
      run += v;
    }
    total_s = run;
    *num_post = run;
  }
  __syncthreads();
  const int start = wsum[wave] + x - pad;
  const int total = total_s;   // <= numel + E (bs - 1) = max_padded
  hist[tid] = tid < E ? start : INT_MAX;
  cursor[tid] = start;
  for (int i = tid; i < max_padded; i += ALIGN_THREADS) sorted_ids[i] = numel;
  __syncthreads();

  // block b belongs to the last expert whose segment starts at or before b bs (the empty experts in
  // front of it start at the same place)
  const int used = total / bs;
  for (int bi = tid; bi < max_blocks; bi += ALIGN_THREADS) {
    int ex = 0;
    if (bi < used) {
      const int pos = bi * bs;
      int lo = 0, hi = E;          // first index with start > pos
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (hist[mid] <= pos) lo = mid + 1; else hi = mid;
      }
      ex = lo - 1;
    }
    expert_ids[bi] = ex;
  }
  for (int i = tid; i < numel; i += ALIGN_THREADS) {
    const int e = topk_ids[i];
    if ((unsigned)e < (unsigned)E) sorted_ids[atomicAdd(&cursor[e], 1)] = i;
  }
}

// ---------------------------------------------------------------------------------------------
// (c) silu_and_mul + 1 x 128 group quantiser
// ---------------------------------------------------------------------------------------------
constexpr int SQ_WAVES = 4;

template <typename T>
__global__ __launch_bounds__(SQ_WAVES * 64) void silu_mul_group_quant_kernel(
    uint8_t* __restrict__ out_q, float* __restrict__ out_s, const T* __restrict__ in, int64_t num_groups,
    int groups_per_row, int64_t s_stride_row, int64_t s_stride_group) {
  constexpr int P = 16, SEGS = 64 / P;               // 16 lanes x 8 elements = one 128-group
  const int lane = threadIdx.x & 63;
  const int l = lane & (P - 1), seg = lane / P;
  const int64_t wave = (int64_t)blockIdx.x * SQ_WAVES + (threadIdx.x >> 6);
  const int64_t step = (int64_t)gridDim.x * SQ_WAVES * SEGS;
  const int64_t d = (int64_t)groups_per_row * MOE_QB;

  // the loop bounds are wave-uniform: every DPP below runs with all 64 lanes enabled
  for (int64_t g0 = wave * SEGS; g0 < num_groups; g0 += step) {
    const int64_t grp = g0 + seg;
    const bool ok = grp < num_groups;
    const int64_t gg = ok ? grp : 0;                 // idle lanes re-read group 0
    const int64_t row = gg / groups_per_row;
    const int64_t gi = gg - row * groups_per_row;
    const T* px = in + row * 2 * d + gi * MOE_QB + l * 8;
    const Vec<T, 8> xv = *reinterpret_cast<const Vec<T, 8>*>(px);
    const Vec<T, 8> yv = *reinterpret_cast<const Vec<T, 8>*>(px + d);
    float f[8];
    float m = 0.f;
    uint32_t lo = 0xffffffffu;                       // smallest non-zero |v| bits, minus one
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      f[j] = silu_mul<T>(xv.v[j], yv.v[j]);
      m = fmaxf(m, fabsf(f[j]));
      if constexpr (!__is_same(T, f16_t)) {          // an f16 is never below 2^-24
        const uint32_t bits = (__float_as_uint(f[j]) & 0x7fffffffu) - 1u;
        lo = bits < lo ? bits : lo;
      }
    }
    m = seg_max<P>(ok ? m : 0.f);
    m = fmaxf(m, 1e-10f);
    const float s = m / 448.0f;
    if (ok && l == 0) out_s[row * s_stride_row + gi * s_stride_group] = s;
    const uint2 q = group_quant8(f, s, lo, -448.0f, 448.0f);
    if (ok) *reinterpret_cast<uint2*>(out_q + row * d + gi * MOE_QB + l * 8) = q;
  }
}

// ---------------------------------------------------------------------------------------------
// (d) moe_sum
// ---------------------------------------------------------------------------------------------
template <typename T, int V>
__global__ __launch_bounds__(256) void moe_sum_kernel(T* __restrict__ out, const T* __restrict__ in,
                                                      int64_t num_tokens, int top_k, int hidden) {
  const int cpr = hidden / V;   // chunks per row
  const int64_t total = num_tokens * cpr;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t t = idx / cpr;
    const int ch = (int)(idx - t * cpr);
    const T* p = in + t * top_k * (int64_t)hidden + ch * V;
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.f;
    for (int k = 0; k < top_k; ++k) {
      const Vec<T, V> v = *reinterpret_cast<const Vec<T, V>*>(p + (int64_t)k * hidden);
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] += to_f32(v.v[j]);
    }
    Vec<T, V> o;
#pragma unroll
    for (int j = 0; j < V; ++j) o.v[j] = from_f32<T>(acc[j]);
    *reinterpret_cast<Vec<T, V>*>(out + t * hidden + ch * V) = o;
  }
}

}  // namespace va

using namespace va;

template <typename T>
static void launch_moe_gemm(void* c, const void* a, const void* b, const float* as, const float* bs,
                            const int32_t* sorted_ids, const int32_t* expert_ids, const int32_t* num_post,
                            const float* topk_w, int nvt, int top_k, int bm, int E, int N, int K, int max_padded,
                            int64_t lda, int64_t b_se, int64_t b_sn, int64_t ldc, int64_t as_sm, int64_t as_sk,
                            int64_t bs_se, int64_t bs_sn, int64_t bs_sk, hipStream_t st) {
  // Waves per strip, measured through "moe_ks" (tools/bench_moe.py, profiles/moe_block_fp8.txt; E 256,
  // top-k 8, block_size_m 16), KS 8 / KS 2 in us at 1 / 16 / 64 tokens:
  //   N 4096 K 7168: 39.8 / 37.1,  484 / 473,  1195 / 1130     N 7168 K 2048: 31.8 / 26.0,  384 / 241,   932 / 583
  //   N  512 K 7168:  8.3 / 19.9, 66.1 / 63.8,  155 / 162      N 7168 K  256: 13.7 /  7.6,  152 / 60.4,  452 / 166
  // KS 2 wins wherever N gives it enough workgroups, also at long K (a wave then streams 28 K blocks
  // instead of 7, and a workgroup writes 64-column rows); KS 8 is kept for narrow outputs with a long
  // K, where four strips per workgroup leave too few workgroups for 256 CUs.  The N threshold lies
  // between the measured 512 and 4096: 1024 is NOT measured.
  if (bm == MOE_TILE_BM) {
    // (a'): one workgroup per (m-block, 128-column tile) of the host-side bound
    const int tiles_n = ceil_div(N, MOE_QB);
    const int vec = (ldc % 8 == 0 && ((((uintptr_t)c) & 15) == 0)) ? 1 : 0;
    hipLaunchKernelGGL((moe_block_gemm_tile_kernel<T>), dim3((unsigned)(ceil_div(max_padded, bm) * tiles_n)),
                       dim3(MOE_TILE_BM * 2), 0, st, (T*)c, (const uint8_t*)a, (const uint8_t*)b, as, bs, sorted_ids,
                       expert_ids, num_post, topk_w, nvt, top_k, E, N, K, max_padded, tiles_n, lda, b_se, b_sn, ldc,
                       as_sm, as_sk, bs_se, bs_sn, bs_sk, vec);
    return;
  }
  const int nkb = K / MOE_QB;
  const int ks = g_moe_ks == 8 || g_moe_ks == 2 ? g_moe_ks : (nkb >= 16 && N <= 1024 ? 8 : 2);
  const int nsg = ceil_div(N, 16 * (MOE_WAVES / ks));
  const int mblocks = ceil_div(max_padded, bm);
#define MG(MT, KS)                                                                                              \
  hipLaunchKernelGGL((moe_block_gemm_kernel<T, MT, KS>), dim3((unsigned)(mblocks * nsg)), dim3(MOE_WAVES * 64), \
                     0, st, (T*)c, (const uint8_t*)a, (const uint8_t*)b, as, bs, sorted_ids, expert_ids,        \
                     num_post, topk_w, nvt, top_k, E, N, K, max_padded, nsg, lda, b_se, b_sn, ldc, as_sm,       \
                     as_sk, bs_se, bs_sn, bs_sk)
  if (bm == 16) { if (ks == 8) MG(1, 8); else MG(1, 2); }
  else { if (ks == 8) MG(4, 8); else MG(4, 2); }
#undef MG
}

extern "C" int vllm_amd_moe_blockwise_gemm(void* c, const void* a, const void* b, const float* a_scales,
                                           const float* b_scales, const int32_t* sorted_token_ids,
                                           const int32_t* expert_ids, const int32_t* num_tokens_post_padded,
                                           const float* topk_weights, int num_valid_tokens, int top_k,
                                           int mul_routed_weight, int block_size_m, int max_num_tokens_padded,
                                           int num_experts, int N, int K,
                                           int64_t lda, int64_t b_stride_e, int64_t b_stride_n, int64_t ldc,
                                           int64_t as_stride_m, int64_t as_stride_k, int64_t bs_stride_e,
                                           int64_t bs_stride_n, int64_t bs_stride_k, int out_dtype, void* stream) {
  const char* op = "moe_blockwise_gemm";
  VA_REQUIRE(num_valid_tokens >= 0 && N >= 0 && K >= 0 && num_experts >= 0, VLLM_AMD_EINVAL, "%s: negative dimension", op);
  VA_REQUIRE(block_size_m == 16 || block_size_m == 64 || block_size_m == MOE_TILE_BM, VLLM_AMD_EUNSUPPORTED,
             "%s: block_size_m = %d must be 16 or 64 (streaming) or 128 (tile)", op, block_size_m);
  VA_REQUIRE(out_dtype == VLLM_AMD_BF16 || out_dtype == VLLM_AMD_F16, VLLM_AMD_EUNSUPPORTED,
             "%s: out dtype must be bfloat16 or float16", op);
  VA_REQUIRE(K > 0 && K % MOE_QB == 0, VLLM_AMD_EUNSUPPORTED,
             "%s: K = %d must be a positive multiple of the 128-wide scale block", op, K);
  VA_REQUIRE(top_k >= 1 && num_valid_tokens % top_k == 0, VLLM_AMD_EINVAL,
             "%s: num_valid_tokens %d is not a multiple of top_k %d", op, num_valid_tokens, top_k);
  if (num_valid_tokens == 0 || N == 0 || num_experts == 0) return VLLM_AMD_OK;
  VA_REQUIRE(c && a && b && a_scales && b_scales && sorted_token_ids && expert_ids && num_tokens_post_padded,
             VLLM_AMD_EINVAL, "%s: null pointer", op);
  VA_REQUIRE(!mul_routed_weight || topk_weights, VLLM_AMD_EINVAL, "%s: mul_routed_weight without topk_weights", op);
  VA_REQUIRE(lda % 16 == 0 && b_stride_n % 16 == 0 && b_stride_e % 16 == 0 && lda >= K && b_stride_n >= K &&
                 (((uintptr_t)a) & 15) == 0 && (((uintptr_t)b) & 15) == 0,
             VLLM_AMD_EUNSUPPORTED, "%s: lda, the weight strides (>= K) and operand pointers must be multiples of 16",
             op);
  VA_REQUIRE(ldc >= N, VLLM_AMD_EINVAL, "%s: ldc < N", op);
  // the bound is the length of sorted_token_ids as moe_align_block_size was given it: with an expert_map
  // the ids are aligned for the GLOBAL expert count, which the local weight tensor does not show
  VA_REQUIRE(max_num_tokens_padded >= num_valid_tokens, VLLM_AMD_EINVAL,
             "%s: max_num_tokens_padded %d < num_valid_tokens %d", op, max_num_tokens_padded, num_valid_tokens);
  const int64_t max_padded = max_num_tokens_padded;
  const int64_t wgs = ((max_padded + block_size_m - 1) / block_size_m) * (int64_t)ceil_div(N, 16);
  VA_REQUIRE(wgs < INT_MAX, VLLM_AMD_EUNSUPPORTED, "%s: too many workgroups", op);
  hipStream_t st = (hipStream_t)stream;
  const float* tw = mul_routed_weight ? topk_weights : nullptr;
  if (out_dtype == VLLM_AMD_BF16)
    launch_moe_gemm<bf16_t>(c, a, b, a_scales, b_scales, sorted_token_ids, expert_ids, num_tokens_post_padded, tw,
                            num_valid_tokens, top_k, block_size_m, num_experts, N, K, (int)max_padded, lda,
                            b_stride_e, b_stride_n, ldc, as_stride_m, as_stride_k, bs_stride_e, bs_stride_n,
                            bs_stride_k, st);
  else
    launch_moe_gemm<f16_t>(c, a, b, a_scales, b_scales, sorted_token_ids, expert_ids, num_tokens_post_padded, tw,
                           num_valid_tokens, top_k, block_size_m, num_experts, N, K, (int)max_padded, lda,
                           b_stride_e, b_stride_n, ldc, as_stride_m, as_stride_k, bs_stride_e, bs_stride_n,
                           bs_stride_k, st);
  VA_LAUNCH_CHECK("moe_blockwise_gemm launch");
  return VLLM_AMD_OK;
}

extern "C" int vllm_amd_moe_align_block_size(const int32_t* topk_ids, int64_t numel, int num_experts,
                                             int block_size, int32_t* sorted_token_ids, int32_t* expert_ids,
                                             int32_t* num_tokens_post_pad, void* stream) {
  const char* op = "moe_align_block_size";
  VA_REQUIRE(numel >= 0 && num_experts >= 0 && block_size > 0, VLLM_AMD_EINVAL, "%s: bad shape", op);
  VA_REQUIRE(num_experts <= ALIGN_THREADS, VLLM_AMD_EUNSUPPORTED, "%s: num_experts %d > %d", op, num_experts,
             ALIGN_THREADS);
  const int64_t max_padded = numel + (int64_t)num_experts * (block_size - 1);
  VA_REQUIRE(max_padded < INT_MAX, VLLM_AMD_EUNSUPPORTED, "%s: numel %lld is too large", op, (long long)numel);
  if (numel == 0) return VLLM_AMD_OK;   // no slot: the GEMM over it is empty as well
  VA_REQUIRE(topk_ids && sorted_token_ids && expert_ids && num_tokens_post_pad, VLLM_AMD_EINVAL, "%s: null pointer",
             op);
  const int max_blocks = (int)((max_padded + block_size - 1) / block_size);
  hipLaunchKernelGGL(moe_align_kernel, dim3(1), dim3(ALIGN_THREADS), 0, (hipStream_t)stream, topk_ids,
                     sorted_token_ids, expert_ids, num_tokens_post_pad, (int)numel, num_experts, block_size,
                     (int)max_padded, max_blocks);
  VA_LAUNCH_CHECK("moe_align_block_size launch");
  return VLLM_AMD_OK;
}

extern "C" int vllm_amd_silu_and_mul_group_quant(void* out_q, float* out_s, const void* input, int64_t num_rows,
                                                 int d, int64_t s_stride_row, int64_t s_stride_group, int dtype,
                                                 void* stream) {
  const char* op = "silu_and_mul_group_quant";
  VA_REQUIRE(num_rows >= 0 && d >= 0, VLLM_AMD_EINVAL, "%s: bad shape", op);
  VA_REQUIRE(d % MOE_QB == 0, VLLM_AMD_EUNSUPPORTED, "%s: intermediate size %d is not a multiple of 128", op, d);
  VA_REQUIRE(dtype == VLLM_AMD_F16 || dtype == VLLM_AMD_BF16, VLLM_AMD_EUNSUPPORTED,
             "%s: input must be float16 or bfloat16", op);
  if (num_rows == 0 || d == 0) return VLLM_AMD_OK;
  VA_REQUIRE(out_q && out_s && input, VLLM_AMD_EINVAL, "%s: null pointer", op);
  VA_REQUIRE((((uintptr_t)input) & 15) == 0 && (((uintptr_t)out_q) & 7) == 0, VLLM_AMD_EUNSUPPORTED,
             "%s: input must be 16-byte and output 8-byte aligned", op);
  const int gpr = d / MOE_QB;
  const int64_t ng = num_rows * gpr;
  const int64_t per_wg = SQ_WAVES * 4;   // groups per workgroup and step
  int64_t grid = (ng + per_wg - 1) / per_wg;
  if (grid > 256 * 8) grid = 256 * 8;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == VLLM_AMD_F16)
    hipLaunchKernelGGL((silu_mul_group_quant_kernel<f16_t>), dim3((unsigned)grid), dim3(SQ_WAVES * 64), 0, st,
                       (uint8_t*)out_q, out_s, (const f16_t*)input, ng, gpr, s_stride_row, s_stride_group);
  else
    hipLaunchKernelGGL((silu_mul_group_quant_kernel<bf16_t>), dim3((unsigned)grid), dim3(SQ_WAVES * 64), 0, st,
                       (uint8_t*)out_q, out_s, (const bf16_t*)input, ng, gpr, s_stride_row, s_stride_group);
  VA_LAUNCH_CHECK("silu_and_mul_group_quant launch");
  return VLLM_AMD_OK;
}

template <typename T>
static void launch_moe_sum(void* out, const void* in, int64_t nt, int top_k, int hidden, hipStream_t st) {
  const bool vec = hidden % 8 == 0 && (((uintptr_t)out | (uintptr_t)in) & 15) == 0;
  const int64_t total = nt * (vec ? hidden / 8 : hidden);
  int64_t grid = (total + 255) / 256;
  if (grid > 256 * 16) grid = 256 * 16;
  if (vec)
    hipLaunchKernelGGL((moe_sum_kernel<T, 8>), dim3((unsigned)grid), dim3(256), 0, st, (T*)out, (const T*)in, nt,
                       top_k, hidden);
  else
    hipLaunchKernelGGL((moe_sum_kernel<T, 1>), dim3((unsigned)grid), dim3(256), 0, st, (T*)out, (const T*)in, nt,
                       top_k, hidden);
}

extern "C" int vllm_amd_moe_sum(void* out, const void* input, int64_t num_tokens, int top_k, int hidden_size,
                                int dtype, void* stream) {
  const char* op = "moe_sum";
  VA_REQUIRE(num_tokens >= 0 && top_k >= 1 && hidden_size >= 0, VLLM_AMD_EINVAL, "%s: bad shape", op);
  VA_REQUIRE(dtype == VLLM_AMD_F16 || dtype == VLLM_AMD_BF16, VLLM_AMD_EUNSUPPORTED,
             "%s: input must be float16 or bfloat16", op);
  if (num_tokens == 0 || hidden_size == 0) return VLLM_AMD_OK;
  VA_REQUIRE(out && input, VLLM_AMD_EINVAL, "%s: null pointer", op);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == VLLM_AMD_F16) launch_moe_sum<f16_t>(out, input, num_tokens, top_k, hidden_size, st);
  else launch_moe_sum<bf16_t>(out, input, num_tokens, top_k, hidden_size, st);
  VA_LAUNCH_CHECK("moe_sum launch");
  return VLLM_AMD_OK;
}
