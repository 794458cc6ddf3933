// Block-scaled w8a8 fp8 (OCP e4m3fn) GEMM for gfx950: 128 x 128 weight scales, 1 x 128
// activation scales ("blockwise scaling like found in DeepSeek V3", vllm/_custom_ops.py:709-723
// of the reference):
//
//   out[m, n] = ( sum_kb As[m, kb] Bs[kb, n / 128] sum_{k in block kb} A[m, k] B[k, n] ).to(out_t)
//               (+ bias[n])
//
// A e4m3 [M, K] row-major, B e4m3 [K, N] column-major (= the [N, K] weight), K % 128 == 0, N
// arbitrary (the last scale column covers a ragged tail).  As / Bs are fp32 and addressed through two
// element strides each, so row-major and token-contiguous activation scales and the transposed view
// of a checkpoint's [N/128, K/128] weight scales are all read in place.
//
// One v_mfma_scale_f32_16x16x128_f8f6f4 (unit E8M0 scales, the 2x-rate fp8 MFMA) consumes exactly one
// 128-byte scale group, so the per-group product is ONE instruction's result: per K block every MFMA
// runs with a zero C operand (an inline constant), and its four results are folded into the fp32
// accumulator with acc = fma(partial, As * Bs, acc).  The product is computed transposed (A operand =
// weight rows, B operand = activation rows): lane (c16, g4) holds 4 consecutive n of output row
// m = c16 of its m-tile, so it needs ONE activation scale per m-tile and K block, and s = As * Bs is
// computed once per (m-tile, K block).
//
// (a) Tile kernel, M > 64: BM x 128 x 128 B tiles, BM = 128 (4 waves) or 256 (8 waves), every wave a
//     64 x 64 sub-tile = 4 x 4 MFMA tiles.  BN is 128 on purpose: a tile is one weight-scale column,
//     so Bs[kb, tn] is workgroup-uniform and comes through a scalar load.  Staging is the skeleton of
//     scaled_mm_large.hip: global_load_lds, 16 B per lane, into an XOR-swizzled [rows][128 B] image
//     (the swizzle is applied to the per-lane SOURCE address and to the read address), a ring of 4
//     (BM 128) or 3 (BM 256) stages, one barrier per K block.  The BM activation scales of a K block
//     are staged WITH its tile: one more LDS-DMA per wave (4 bytes per lane) into a strip next to the
//     stage, so the only vector-memory instructions of the loop are LDS-DMA, every wave issues the same
//     number per stage, and the one hand-counted wait -- vmcnt((NST - 2) * loads per stage) in front of
//     the barrier -- stays provable.  Per block: that wait -> barrier -> request ALL fragments and the
//     lane's 4 scales (inline-asm ds_read, 17 per lane) -> issue the DMA of block kb + NST - 1 ->
//     lgkmcnt(0) -> 16 MFMAs + 64 FMAs.  Bs is a scalar load whose wait is the compiler's.  There
//     is no hand-built ring of partials and no fragment-level pipeline: the partials are independent
//     registers, so the compiler's scheduler MAY place the FMAs of one MFMA tile under the next MFMA,
//     but how far it does was not measured, and the block's reads -> wait -> math chain is serial
//     (open items).  The output goes through LDS (overlaying the stages) so that stores
//     write whole 16-byte pieces of rows.
// (b) Weight-streaming kernel, M <= 64 (decode): bound by the N x K weight bytes.  A workgroup of 8
//     waves owns 16 output columns and all M rows (1, 2 or 4 MFMA tiles); the
//     waves take the K blocks round-robin.  Weight and activation fragments go straight from global
//     memory to VGPRs in MFMA operand order with the K permutation of scaled_mm_skinny_kernel (lane
//     group g takes bytes 64 j + 16 g: one load instruction reads 16 rows x 64 contiguous bytes),
//     four K blocks of loads in flight per wave.  Per block partial = mfma(w, a, 0), acc += partial *
//     (As[m, kb] * Bs[kb, n0 / 128]).  The 8 partial sums meet in LDS; bias, cast, store.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage, bf16 out):
//   tile BM 128: 164 VGPRs + 20 AGPRs, scratch 0, LDS 133120 B, 1 workgroup (4 waves) / CU
//   tile BM 256: 202 VGPRs, 0 AGPRs, scratch 0, LDS 150528 B, 1 workgroup (8 waves) / CU
//   stream MT 1 / 2 / 4: 94 / 148 / 146 VGPRs, scratch 0, LDS 8704 / 17408 / 34816 B, occupancy 5 / 3 / 3
// Nothing is allocated or synchronised and there is no workspace: graph-capturable.
#include "common.cuh"

namespace va {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) int i32x8;

constexpr int QB = 128;   // scale block edge = K bytes per MFMA = tile columns

int g_mm_block_kernel = 0;   // tuning "mm_block_kernel": 0 = by M, 1 = always the tile kernel, 2 / 3 = its 128- / 256-row form

__device__ __forceinline__ int qswz(int row) {
  return ((row >> 1) & 1) | (((row >> 2) & 1) << 2);
}

// the product of one 128-byte K block: C operand zero
__device__ __forceinline__ f32x4 block_mfma(i32x8 w, i32x8 a) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, a, (f32x4){0.f, 0.f, 0.f, 0.f}, 0 /*fp8 e4m3*/, 0, 0,
                                                          0x7f7f7f7f, 0, 0x7f7f7f7f);
}
__device__ __forceinline__ i32x8 frag8(uint4 lo, uint4 hi) {
  return (i32x8){(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
}

// LDS reads of the tile kernel's K loop as inline asm: a C++ LDS load is ordered by hipcc behind ALL
// outstanding LDS-DMA (s_waitcnt vmcnt(0)), which would serialise the ring with the math
typedef __attribute__((ext_vector_type(4))) int i32x4;
template <int OFF>
__device__ __forceinline__ i32x4 lds_read16(uint32_t addr) {
  i32x4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}
template <int OFF>
__device__ __forceinline__ float lds_read4(uint32_t addr) {
  float v;
  asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}

// ---------------------------------------------------------------------------------------------
// (a) tile kernel
// ---------------------------------------------------------------------------------------------
template <typename out_t, int BM>
__global__ __launch_bounds__(BM * 2) void scaled_mm_block_tile_kernel(
    out_t* __restrict__ out, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
    const float* __restrict__ a_scales, const float* __restrict__ b_scales, const out_t* __restrict__ bias, int M,
    int N, int K, int64_t lda, int64_t ldb, int64_t ldc, int64_t as_sm, int64_t as_sk, int64_t bs_sk, int64_t bs_sn,
    int vec_store) {
  constexpr int NW = BM / 32;                        // waves: (BM / 64) x 2, each 64 x 64
  constexpr int A_BYTES = BM * QB, W_BYTES = QB * QB, STAGE = A_BYTES + W_BYTES;
  constexpr int RPR = 8 * NW;                        // rows staged per glds round
  constexpr int A_ROUNDS = BM / RPR, W_ROUNDS = QB / RPR;
  constexpr int OROW = QB + 8;                       // output image: row stride in elements (272 B)
  constexpr int NST = BM == 128 ? 4 : 3;             // ring stages: NST - 1 K blocks in flight
  constexpr int STRIP = BM * 4;                      // the BM activation scales of a K block
  constexpr int PER = A_ROUNDS + W_ROUNDS + 1;       // LDS-DMA instructions per lane and stage
  static_assert(BM * OROW * (int)sizeof(out_t) <= NST * STAGE, "the output image overlays the stages");
  static_assert(NST * (STAGE + STRIP) <= 160 * 1024 && (NST - 2) * PER <= 63, "LDS size, vmcnt is 6 bits");
  __shared__ __attribute__((aligned(16))) uint8_t lds[NST * (STAGE + STRIP)];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c16 = lane & 15, g4 = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;

  // hardware workgroup i runs on XCD i % 8: give every XCD a contiguous run of tiles, m fastest, so
  // that the tiles sharing a weight panel share an L2
  const int tiles_m = (M + BM - 1) / BM, tiles_n = (N + QB - 1) / QB;
  int wg = blockIdx.x;
  {
    const int nwg = tiles_m * tiles_n;
    const int q = nwg / 8, r = nwg % 8, xcd = wg % 8, idx = wg / 8;
    wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const int tm = wg % tiles_m, tn = wg / tiles_m;
  const int m0 = tm * BM, n0 = tn * QB;

  // staging: in round r wave w fills rows [RPR r + 8 w, +8); lane -> (row = lane >> 3, slot = lane & 7)
  // loads logical chunk slot ^ f(row), so the lane-linear LDS image is the swizzled tile.  Rows past
  // M / N re-read the last valid row: their outputs are never stored.
  const int srow = lane >> 3, sslot = lane & 7;
  const uint8_t* a_src[A_ROUNDS];
  const uint8_t* w_src[W_ROUNDS];
#pragma unroll
  for (int r = 0; r < A_ROUNDS; ++r) {
    const int row = RPR * r + 8 * wave + srow;
    const int m = min(m0 + row, M - 1);
    a_src[r] = a + (int64_t)m * lda + ((sslot ^ qswz(row)) << 4);
  }
#pragma unroll
  for (int r = 0; r < W_ROUNDS; ++r) {
    const int row = RPR * r + 8 * wave + srow;
    const int n = min(n0 + row, N - 1);
    w_src[r] = b + (int64_t)n * ldb + ((sslot ^ qswz(row)) << 4);
  }
  // the activation scales of a K block travel with its tile: every wave copies 64 of the BM values
  // As[m0 + row, kb] into the stage's strip with one 4-byte LDS-DMA (waves beyond BM / 64 repeat the
  // rows of wave % (BM / 64): the same values to the same place, so every wave counts PER loads)
  const int strip_row = (wave % (BM / 64)) * 64;
  const float* as_src = a_scales + (int64_t)min(m0 + strip_row + lane, M - 1) * as_sm;
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
  const float* bs_ptr = b_scales + (int64_t)tn * bs_sn;   // workgroup-uniform

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
    const int ch = ((2 * g4 + j) ^ qswz(c16)) << 4;
    w_addr[j] = lds_base + A_BYTES + (wn * 64 + c16) * QB + ch;
    a_addr[j] = lds_base + (wm * 64 + c16) * QB + ch;
  }
  const uint32_t s_addr = lds_base + NST * STAGE + (wm * 64 + c16) * 4;

  // Ring of NST stages, NST - 1 K blocks in flight.  Per block: wait for the own LDS-DMA of block kb
  // (everything but the NST - 2 younger stages; near the end fewer are in flight, so drain) ->
  // s_barrier (everybody's has landed, and everybody is past its reads of the stage refilled next) ->
  // request all fragments and the four scales of the block -> issue the DMA of block kb + NST - 1 ->
  // lgkmcnt(0) -> 16 MFMAs with a zero C operand, each folded into the accumulators by 4 FMAs.
  const int nk = K / QB;
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
      wl[t] = lds_read16<t * 16 * QB>(wa0);
      wh[t] = lds_read16<t * 16 * QB>(wa1);
      al[t] = lds_read16<t * 16 * QB>(aa0);
      ah[t] = lds_read16<t * 16 * QB>(aa1);
      as[t] = lds_read4<t * 64>(sa);
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
        const f32x4 p = block_mfma(wf[nt], af);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[nt][mt][r] = fmaf(p[r], s, acc[nt][mt][r]);
      }
    }
  }

  // ---- epilogue: lane holds C^T[n = 16 nt + 4 g4 + r][m = 16 mt + c16]; through LDS, whole rows out
  __syncthreads();   // everybody is past its fragment reads
  out_t* ot = reinterpret_cast<out_t*>(lds);
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int nl = wn * 64 + nt * 16 + 4 * g4;
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (bias) {
#pragma unroll
      for (int r = 0; r < 4; ++r) bv[r] = to_f32(bias[min(n0 + nl + r, N - 1)]);
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int ml = wm * 64 + mt * 16 + c16;
      struct alignas(8) V4 { out_t e[4]; } pk;
#pragma unroll
      for (int r = 0; r < 4; ++r) pk.e[r] = from_f32<out_t>(acc[nt][mt][r] + bv[r]);
      *reinterpret_cast<V4*>(ot + ml * OROW + nl) = pk;
    }
  }
  __syncthreads();
  const int chunk = tid & 15;            // 8 output elements = 16 B
  const int n = n0 + chunk * 8;
  for (int row = tid >> 4; row < BM; row += NW * 4) {
    const int m = m0 + row;
    if (m >= M || n >= N) continue;
    const uint4 v = *reinterpret_cast<const uint4*>(ot + row * OROW + chunk * 8);
    out_t* op = out + (int64_t)m * ldc + n;
    if (vec_store && n + 8 <= N) {
      *reinterpret_cast<uint4*>(op) = v;
    } else {
      const out_t* e = reinterpret_cast<const out_t*>(&v);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (n + j < N) op[j] = e[j];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// (b) weight-streaming kernel
// ---------------------------------------------------------------------------------------------
constexpr int QS_WAVES = 8;

template <typename out_t, int MT>
__global__ __launch_bounds__(QS_WAVES * 64) void scaled_mm_block_stream_kernel(
    out_t* __restrict__ out, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
    const float* __restrict__ a_scales, const float* __restrict__ b_scales, const out_t* __restrict__ bias, int M,
    int N, int K, int64_t lda, int64_t ldb, int64_t ldc, int64_t as_sm, int64_t as_sk, int64_t bs_sk,
    int64_t bs_sn) {
  __shared__ float red[QS_WAVES][MT][16][17];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c16 = lane & 15, g4 = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const int nkb = K / QB;

  // rows past N / M re-read the last valid row: their outputs are never stored
  const uint8_t* wrow = b + (int64_t)min(n0 + c16, N - 1) * ldb + 16 * g4;
  const uint8_t* arow[MT];
  const float* as_ptr[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = min(t * 16 + c16, M - 1);
    arow[t] = a + (int64_t)m * lda + 16 * g4;
    as_ptr[t] = a_scales + (int64_t)m * as_sm;
  }
  const float* bs_ptr = b_scales + (int64_t)(n0 / QB) * bs_sn;   // 16 | 128: one scale column per workgroup

  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  constexpr int UN = MT <= 2 ? 4 : 2;   // K blocks of loads in flight per wave
  for (int kb = wave; kb < nkb; kb += UN * QS_WAVES) {
    uint4 wv[UN][2], av[UN][MT][2];
    float as[UN][MT], bs[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int kbu = kb + u * QS_WAVES;       // wave-uniform
      if (kbu < nkb) {
        const int64_t k = (int64_t)kbu * QB;   // + 16 g4 is in the row pointers
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
      if (kb + u * QS_WAVES < nkb) {
        const i32x8 wf = frag8(wv[u][0], wv[u][1]);
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          const f32x4 p = block_mfma(wf, frag8(av[u][t][0], av[u][t][1]));
          const float s = as[u][t] * bs[u];
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[t][r] = fmaf(p[r], s, acc[t][r]);
        }
      }
    }
  }
  // lane holds C^T[n = 4 g4 + r][m = 16 t + c16]
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][t][c16][4 * g4 + r] = acc[t][r];   // [m][n]
  __syncthreads();
  for (int idx = threadIdx.x; idx < MT * 256; idx += QS_WAVES * 64) {
    const int t = idx >> 8, mm = (idx >> 4) & 15, nn = idx & 15;
    const int m = t * 16 + mm, no = n0 + nn;
    if (m >= M || no >= N) continue;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < QS_WAVES; ++w) v += red[w][t][mm][nn];
    if (bias) v += to_f32(bias[no]);
    out[(int64_t)m * ldc + no] = from_f32<out_t>(v);
  }
}

}  // namespace va

using namespace va;

template <typename T>
static void launch_block_mm(void* out, const void* a, const void* b, const float* as, const float* bs,
                            const void* bias, int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc,
                            int64_t as_sm, int64_t as_sk, int64_t bs_sk, int64_t bs_sn, hipStream_t st) {
  // (b) wherever it applies, M <= 64 = four MFMA tiles: measured through "mm_block_kernel"
  // (tools/bench_block_gemm.py, profiles/block_fp8_gemm.txt), tile vs streaming kernel in us:
  //   1536 x 7168: M 16 46.8 / 10.7, M 32 47.0 / 15.7, M 48 47.3 / 21.2, M 64 47.5 / 24.8
  //   7168 x 2304: M 16 18.1 /  7.0, M 32 18.3 / 10.8, M 48 18.6 / 14.0, M 64 18.8 / 15.9
  // (the tile kernel is flat in M here: its K loop is latency-bound)
  const bool stream = g_mm_block_kernel == 0 && M <= 64;
  if (stream) {
    const int mt = ceil_div(M, 16);
#define QS(MT)                                                                                                   \
  hipLaunchKernelGGL((scaled_mm_block_stream_kernel<T, MT>), dim3(ceil_div(N, 16)), dim3(QS_WAVES * 64), 0, st,  \
                     (T*)out, (const uint8_t*)a, (const uint8_t*)b, as, bs, (const T*)bias, M, N, K, lda, ldb,   \
                     ldc, as_sm, as_sk, bs_sk, bs_sn)
    if (mt == 1) QS(1); else if (mt == 2) QS(2); else QS(4);
#undef QS
    return;
  }
  // 256-row tiles once they still give about 3/4 of a round of workgroups on 256 CUs, 128-row tiles
  // otherwise (both forms run one workgroup per CU).  The threshold is the rule of launch_scaled_mm
  // carried over, NOT measured for these kernels: no A/B of the two forms is recorded yet
  // ("mm_block_kernel" 2 / 3 force them).
  const int tn = ceil_div(N, QB);
  const int vec = (ldc % 8 == 0 && ((((uintptr_t)out) & 15) == 0)) ? 1 : 0;
  const bool big = g_mm_block_kernel == 3 || (g_mm_block_kernel != 2 && ceil_div(M, 256) * tn >= 190);
#define QT(BM)                                                                                                   \
  hipLaunchKernelGGL((scaled_mm_block_tile_kernel<T, BM>), dim3(ceil_div(M, BM) * tn), dim3(BM * 2), 0, st,      \
                     (T*)out, (const uint8_t*)a, (const uint8_t*)b, as, bs, (const T*)bias, M, N, K, lda, ldb,   \
                     ldc, as_sm, as_sk, bs_sk, bs_sn, vec)
  if (big) QT(256); else QT(128);
#undef QT
}

extern "C" int vllm_amd_scaled_mm_blockwise(void* out, const void* a, const void* b, const float* a_scales,
                                            const float* b_scales, const void* bias, int M, int N, int K,
                                            int64_t lda, int64_t ldb, int64_t ldc, int64_t as_stride_m,
                                            int64_t as_stride_k, int64_t bs_stride_k, int64_t bs_stride_n,
                                            int out_dtype, void* stream) {
  const char* op = "scaled_mm_blockwise";
  VA_REQUIRE(M >= 0 && N >= 0 && K >= 0, VLLM_AMD_EINVAL, "%s: negative dimension", op);
  if (M == 0 || N == 0) return VLLM_AMD_OK;
  VA_REQUIRE(out && a && b && a_scales && b_scales, VLLM_AMD_EINVAL, "%s: null pointer", op);
  VA_REQUIRE(out_dtype == VLLM_AMD_BF16 || out_dtype == VLLM_AMD_F16, VLLM_AMD_EUNSUPPORTED,
             "%s: out dtype must be bfloat16 or float16", op);
  VA_REQUIRE(K > 0 && K % QB == 0, VLLM_AMD_EUNSUPPORTED,
             "%s: K = %d must be a positive multiple of the 128-wide scale block", op, K);
  VA_REQUIRE(lda % 16 == 0 && ldb % 16 == 0 && lda >= K && ldb >= K && (((uintptr_t)a) & 15) == 0 &&
                 (((uintptr_t)b) & 15) == 0,
             VLLM_AMD_EUNSUPPORTED, "%s: lda, ldb (>= K) and operand pointers must be multiples of 16", op);
  VA_REQUIRE(ldc >= N, VLLM_AMD_EINVAL, "%s: ldc < N", op);
  hipStream_t st = (hipStream_t)stream;
  if (out_dtype == VLLM_AMD_BF16)
    launch_block_mm<bf16_t>(out, a, b, a_scales, b_scales, bias, M, N, K, lda, ldb, ldc, as_stride_m, as_stride_k,
                            bs_stride_k, bs_stride_n, st);
  else
    launch_block_mm<f16_t>(out, a, b, a_scales, b_scales, bias, M, N, K, lda, ldb, ldc, as_stride_m, as_stride_k,
                           bs_stride_k, bs_stride_n, st);
  VA_LAUNCH_CHECK("scaled_mm_blockwise launch");
  return VLLM_AMD_OK;
}
