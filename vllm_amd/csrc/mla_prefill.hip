// MLA prefill attention: ragged (varlen) flash attention forward with a q.k width of 192 and a v width of 128, plus
// merge_attn_states.  Replaces what MLACommonImpl._forward_prefill / _compute_prefill_context
// (vllm/v1/attention/backends/mla/common.py:1017-1127) do with torch.cat + a padded v + flash_attn_varlen_func and
// the Triton merge kernel (vllm/attention/ops/triton_merge_attn_states.py:12-97).
//
// The attention kernel keeps the scheme of prefill_fa.hip and changes what the MLA shapes change:
//   * a workgroup = 8 waves = 256 query tokens of ONE (sequence, head) -- there is no GQA group to pack, every head
//     has its own K / V; a wave owns 32 tokens and computes with v_mfma_f32_32x32x16 on the transposed problem:
//     S^T[n, m] = K[n, :] . Q[m, :] (A = K rows from LDS, B = Q^T in 48 registers, 12 k-steps),
//     O^T[d, m] += V^T[d, n] . P^T[n, m] (A = V^T by the transposing LDS read, B = P^T, which never leaves the
//     registers), O^T 64 accumulator registers;
//   * K arrives in SPLIT form and is staged in split form: the 128 "nope" columns of a key (a strided view of the
//     up-projection's [Tk, H, 256] output) into a [64][128] image, the 64 rope columns (k_pe, head stride 0 when one
//     rope key serves all heads) into a [64][64] image of its own.  Each image has a row length that is a power of two,
//     so each keeps a conflict-free XOR swizzle (16-byte chunk ^= key & 15, resp. ^= (key >> 1) & 7: rows of 128 bytes
//     alternate between the two halves of the banks); k-steps 0-7 read the first image, 8-11 the second.  No
//     concatenated or padded copy of K or V exists anywhere;
//   * 64-key tiles, double-buffered: (16 + 8) KiB of K and 16 KiB of V per tile, 80 KiB of LDS, one barrier per tile;
//     registers hold tile t + 1 while tile t is computed, waves 4-7 stage in front of their compute and waves 0-3
//     behind it;
//   * lazy running maximum (rescale only when a tile maximum exceeds it by more than 2^8);
//   * causal launches are bottom-right aligned (query i of Sq sees keys j <= i + Sk - Sq); a wave computes its
//     interior tiles without a mask, applies the mask (in the MFMA's C operand) on its diagonal tiles and on the
//     sequence's last, partial tile, and only helps staging above its rows; the workgroup stops at its last visible tile;
//   * launch order: hardware workgroup ids are remapped so that every XCD gets a contiguous range of logical ids with
//     the row blocks of one (sequence, head) adjacent, then the heads: the row blocks of a head read the SAME K / V
//     rows (all of them, up to the diagonal), neighbouring heads share only k_pe (a fifth of the bytes), so it is
//     the row blocks that should meet in one L2.  Row blocks are taken last first: under the causal mask the last
//     block of a sequence is its heaviest.
//   * optional lse [H, Tq] (natural log), the layout merge_attn_states reads; a row without a visible key gets
//     out = 0 and lse = -inf.
#include "mma.cuh"

#include <math.h>

namespace va {
namespace mlap {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

template <typename T> struct Mma32;
template <> struct Mma32<bf16_t> {
  static __device__ __forceinline__ f32x16 mfma(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c,
                                                   0, 0, 0);
  }
};
template <> struct Mma32<f16_t> {
  static __device__ __forceinline__ f32x16 mfma(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c,
                                                  0, 0, 0);
  }
};

constexpr int NW = 8, BM = 32 * NW, BN = 64;      // waves, query rows, keys per tile
constexpr int DN = 128, DP = 64, DV = 128;        // nope / rope columns of k, columns of v
constexpr int KS = (DN + DP) / 16, KSN = DN / 16, DB = DV / 32;
constexpr int KN_ROWB = 2 * DN, KP_ROWB = 2 * DP, V_ROWB = 2 * DV;
constexpr int KN_TILE = BN * KN_ROWB, KP_TILE = BN * KP_ROWB, V_TILE = BN * V_ROWB;   // 16 + 8 + 16 KiB
constexpr int KN_OFF = 0, KP_OFF = 2 * KN_TILE, V_OFF = KP_OFF + 2 * KP_TILE;
constexpr int LDS_BYTES = V_OFF + 2 * V_TILE;     // 80 KiB
constexpr int KR = 8, VR = 4;                     // fragment reads in flight
constexpr float THR = 8.f;                        // lazy rescale threshold (log2 domain)

struct Params {
  void* o; float* lse;
  const void *q, *k_nope, *k_pe, *v;
  const int *cu_q, *cu_k;
  int num_seqs, blocks_per_seq, causal;
  float sm_scale;
  int64_t q_st, q_sh, o_st, o_sh, kn_st, kn_sh, kp_st, kp_sh, v_st, v_sh, lse_sh;
};

__device__ __forceinline__ float max3(float a, float b, float c) {
  float r;   // (fmaxf on MFMA results makes hipcc canonicalise every input first)
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
// own value and the value of lane ^ 32, in some order (see prefill_fa.hip)
__device__ __forceinline__ void swap32(float& a, float& b) {
  asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ float xmax(float x) { float a = x, b = x; swap32(a, b); return fmaxf(a, b); }
__device__ __forceinline__ float xsum(float x) { float a = x, b = x; swap32(a, b); return a + b; }
__device__ __forceinline__ u32x2 lds_tr16(const uint8_t* p) {
  typedef __attribute__((ext_vector_type(4))) short s16x4;
  const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
  return __builtin_bit_cast(u32x2, v);
}

template <typename T>
__global__ __launch_bounds__(64 * NW) void mla_prefill_kernel(const Params p) {
  __shared__ __attribute__((aligned(1024))) uint8_t lds[LDS_BYTES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l32 = lane & 31, hi = lane >> 5;

  // ---- workgroup -> (row block of some sequence, head): XCD-contiguous logical ids, row blocks fastest, last first
  int wg = blockIdx.x + gridDim.x * blockIdx.y;
  {
    const int nwg = gridDim.x * gridDim.y;
    const int q8 = nwg / 8, r8 = nwg % 8, xcd = wg % 8, idx = wg / 8;
    wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
  }
  const int g = gridDim.x - 1 - wg % gridDim.x;
  const int head = wg / gridDim.x;
  // grid.x enumerates the row blocks of all sequences: blocks_per_seq each (the host found that the smaller grid), or
  // packed, with sequence i starting at block cu_q[i] / BM + i (num_tokens / BM + num_seqs bounds the count)
  int seq = 0;
  if (p.blocks_per_seq > 0) {
    seq = g / p.blocks_per_seq;
  } else {
    int lo = 0, hi2 = p.num_seqs;
    while (hi2 - lo > 1) {
      const int mid = (lo + hi2) >> 1;
      if (p.cu_q[mid] / BM + mid <= g) lo = mid; else hi2 = mid;
    }
    seq = lo;
  }
  const int tok0 = p.cu_q[seq], qlen = p.cu_q[seq + 1] - tok0;
  const int key0 = p.cu_k[seq], klen = p.cu_k[seq + 1] - key0;
  const int tok_base = (p.blocks_per_seq > 0 ? g % p.blocks_per_seq : g - (tok0 / BM + seq)) * BM;
  if (tok_base >= qlen) return;
  const int new_end = min(tok_base + BM, qlen);
  const int off = klen - qlen;                       // causal: query i sees keys <= i + off

  // ---- this lane's query row --------------------------------------------------------------------------------------
  const int rtok = tok_base + 32 * wave + l32;
  const bool rok = rtok < qlen;
  const int bound = rok ? (p.causal ? rtok + off : klen - 1) : -1;   // last visible key (< 0: none)
  // Q^T fragments (B operand of S^T): column m = this row, k = d = 16 ks + 8 hi + (0..7)
  u32x4 qf[KS];
  {
    const T* qp = (const T*)p.q + (int64_t)(tok0 + (rok ? rtok : 0)) * p.q_st + (int64_t)head * p.q_sh + 8 * hi;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(qp + 16 * ks);
      qf[ks] = rok ? v : (u32x4){0, 0, 0, 0};
    }
  }
  // wave-uniform: the bounds of the wave's first and last row
  const bool w_rows = tok_base + 32 * wave < qlen;
  const int w_last = min(tok_base + 32 * wave + 31, new_end - 1);
  const int w_lo = p.causal ? tok_base + 32 * wave + off : klen - 1;
  const int w_hi = p.causal ? w_last + off : klen - 1;
  const float sc2 = p.sm_scale * kLog2e;             // > 0 (the host checks sm_scale)

  // the workgroup's tiles end at its last row's bound
  const int vis = min(klen, p.causal ? new_end + off : klen);
  const int ntiles = vis > 0 ? (vis + BN - 1) / BN : 0;

  // ---- staging: thread -> (key tid / 8 of the tile, 32 bytes of nope, 16 bytes of rope, 32 bytes of v) --------------
  const int skey = tid >> 3, spiece = tid & 7;
  u32x4 knst[2], kpst, vst[2];
  const T* kn_src = (const T*)p.k_nope + (int64_t)head * p.kn_sh + 16 * spiece;
  const T* kp_src = (const T*)p.k_pe + (int64_t)head * p.kp_sh + 8 * spiece;
  const T* v_src = (const T*)p.v + (int64_t)head * p.v_sh + 16 * spiece;
  auto ld16 = [](const void* ptr) __attribute__((always_inline)) { return *reinterpret_cast<const u32x4*>(ptr); };
  auto issue_loads = [&](int t) __attribute__((always_inline)) {
    const int64_t row = key0 + min(t * BN + skey, klen - 1);   // (keys past the sequence: a clamped address, zeroed below)
    const T* kn = kn_src + row * p.kn_st;
    const T* kp = kp_src + row * p.kp_st;
    const T* vv = v_src + row * p.v_st;
    knst[0] = ld16(kn); knst[1] = ld16(kn + 8);
    kpst = ld16(kp);
    vst[0] = ld16(vv); vst[1] = ld16(vv + 8);
  };
  // images: nope chunk ^= key & 15 (conflict-free ds_read_b128 of 32 keys x one chunk); rope chunk ^= (key >> 1) & 7;
  // V chunk ^= (key & 3) << 2 (the four keys of a transposing read land in four different 64-byte bank ranges)
  uint8_t* kn_wr = lds + KN_OFF + skey * KN_ROWB;
  uint8_t* kp_wr = lds + KP_OFF + skey * KP_ROWB + ((spiece ^ ((skey >> 1) & 7)) << 4);
  uint8_t* v_wr = lds + V_OFF + skey * V_ROWB;
  const int kc0 = ((2 * spiece) ^ (skey & 15)) << 4, kc1 = ((2 * spiece + 1) ^ (skey & 15)) << 4;
  const int vc0 = ((2 * spiece) ^ ((skey & 3) << 2)) << 4, vc1 = ((2 * spiece + 1) ^ ((skey & 3) << 2)) << 4;
  auto write_tile = [&](int t) __attribute__((always_inline)) {
    const int b = t & 1;
    // rows past the sequence are zeroed: their scores are 0 + the mask's -inf, their probabilities 0, and V rows
    // must not hold a NaN (0 * NaN)
    const bool live = t * BN + skey < klen;
    const u32x4 z = {0, 0, 0, 0};
    *reinterpret_cast<u32x4*>(kn_wr + b * KN_TILE + kc0) = live ? knst[0] : z;
    *reinterpret_cast<u32x4*>(kn_wr + b * KN_TILE + kc1) = live ? knst[1] : z;
    *reinterpret_cast<u32x4*>(kp_wr + b * KP_TILE) = live ? kpst : z;
    *reinterpret_cast<u32x4*>(v_wr + b * V_TILE + vc0) = live ? vst[0] : z;
    *reinterpret_cast<u32x4*>(v_wr + b * V_TILE + vc1) = live ? vst[1] : z;
  };

  // ---- fragment read offsets: one per image, the k-step / d block is XORed in at the read (the images are aligned
  // to their row length, so the XOR never carries) -------------------------------------------------------------------
  const int kn_off0 = KN_OFF + l32 * KN_ROWB + ((hi ^ (l32 & 15)) << 4);          // K rows l32 (+ 32 kb), chunk 2 ks + hi
  const int kp_off0 = KP_OFF + l32 * KP_ROWB + ((hi ^ ((l32 >> 1) & 7)) << 4);
  // transposing read: the 16 lanes of group G = lane >> 4 read keys 4 hi + (0..3) (+ 16 g16 + 8 e) x d
  // 32 db + 16 (G & 1) + (0..15); lane 4 q + pp of the group addresses key q, d 4 pp .. 4 pp + 3 and receives
  // d = 32 db + (lane & 31) of the four keys
  const int v_off0 = V_OFF + (4 * hi + ((lane & 15) >> 2)) * V_ROWB +
                     ((4 * ((lane & 15) >> 2) + 2 * ((lane >> 4) & 1) + ((lane & 3) >> 1)) << 4) + 8 * (lane & 1);

  float m_run = -INFINITY, l_run = 0.f;
  f32x16 o[DB];   // O^T[d = 32 db + (r & 3) + 8 (r >> 2) + 4 hi][this row]
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[db][r] = 0.f;

  // ---- one K / V tile: fragment reads run a ring ahead of the MFMAs, the row maximum of key block 0 is taken between
  // the MFMAs of block 1, the probabilities of key group g + 1 between the PV MFMAs of group g (prefill_fa.hip) -------
  auto compute = [&](int t, auto masked_c) __attribute__((always_inline)) {
    constexpr bool MASKED = decltype(masked_c)::value;
    const int bound0 = bound - t * BN;
    const int knofs = (t & 1) * KN_TILE, kpofs = (t & 1) * KP_TILE, vofs = (t & 1) * V_TILE;
    f32x16 s[2];
    u32x4 pb[4];   // P^T fragments of key groups 16 g16 ..: slots 0-3 = keys 4 hi + (0..3), 4-7 = 8 + 4 hi + (0..3)
    u32x4 kf[KR];
    auto k_read = [&](auto ic) __attribute__((always_inline)) {
      constexpr int i = decltype(ic)::value, kb = i / KS, ks = i % KS;   // read i -> (key block, k-step)
      if constexpr (ks < KSN)
        return *reinterpret_cast<const u32x4*>(lds + ((kn_off0 ^ (ks << 5)) + knofs + kb * 32 * KN_ROWB));
      else
        return *reinterpret_cast<const u32x4*>(lds + ((kp_off0 ^ ((ks - KSN) << 5)) + kpofs + kb * 32 * KP_ROWB));
    };
    static_for<KR>([&](auto ic) { kf[decltype(ic)::value] = k_read(ic); });
    __builtin_amdgcn_sched_barrier(0);
    float mx = 0.f;   // maximum of the tile's raw scores in this lane
    static_for<2 * KS>([&](auto ic) {
      constexpr int i = decltype(ic)::value, kb = i / KS, ks = i % KS;
      const u32x4 f = kf[i % KR];
      if constexpr (i + KR < 2 * KS) kf[i % KR] = k_read(std::integral_constant<int, i + KR>{});
      if constexpr (ks == 0) {
        // the accumulator starts at 0, or at -inf where the key is invisible to this row
        f32x16 z;
        const int lim = bound0 - 32 * kb - 4 * hi;
#pragma unroll
        for (int r = 0; r < 16; ++r) z[r] = (!MASKED || (r & 3) + 8 * (r >> 2) <= lim) ? 0.f : -INFINITY;
        s[kb] = Mma32<T>::mfma(f, qf[0], z);
      } else {
        s[kb] = Mma32<T>::mfma(f, qf[ks], s[kb]);
      }
      if constexpr (kb == 1 && ks < 8) {   // block 0 is complete: its maximum, two scores per MFMA
        if constexpr (ks == 0) mx = max3(s[0][0], s[0][1], s[0][1]);
        else mx = max3(mx, s[0][2 * ks], s[0][2 * ks + 1]);
      }
      __builtin_amdgcn_sched_barrier(0);
    });
    u32x4 vf[VR];
    auto v_read = [&](auto ic) __attribute__((always_inline)) {
      constexpr int i = decltype(ic)::value;   // MFMA i -> (key group i / DB, d block i % DB)
      const uint8_t* vp = lds + ((v_off0 ^ ((i % DB) << 6)) + vofs);
      const u32x2 va = lds_tr16(vp + (16 * (i / DB)) * V_ROWB);
      const u32x2 vb = lds_tr16(vp + (16 * (i / DB) + 8) * V_ROWB);
      return (u32x4){va[0], va[1], vb[0], vb[1]};
    };
    static_for<VR>([&](auto ic) { vf[decltype(ic)::value] = v_read(ic); });
    __builtin_amdgcn_sched_barrier(0);
    // lane holds S^T[key = 64 t + 32 kb + (r & 3) + 8 (r >> 2) + 4 hi][this row]
#pragma unroll
    for (int r = 0; r < 16; r += 2) mx = max3(mx, s[1][r], s[1][r + 1]);
    const float ms = xmax(mx) * sc2;
    if (__any(ms > m_run + THR)) {
      const float m_new = fmaxf(m_run, ms);
      const float alpha = m_new == -INFINITY ? 1.f : fast_exp2(m_run - m_new);
      m_run = m_new;
      l_run *= alpha;
#pragma unroll
      for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
    }
    const float msub = m_run == -INFINITY ? 0.f : m_run;
    float psum = 0.f;
    auto p_word = [&](auto gc, auto jc) __attribute__((always_inline)) {   // word j2 of pb[g16]: two probabilities
      constexpr int g16 = decltype(gc)::value, j2 = decltype(jc)::value, r0 = 8 * (g16 & 1) + 2 * j2;
      const float e0 = fast_exp2(fmaf(s[g16 >> 1][r0], sc2, -msub));
      const float e1 = fast_exp2(fmaf(s[g16 >> 1][r0 + 1], sc2, -msub));
      psum += e0;
      psum += e1;
      pb[g16][j2] = Mma<T>::pack2(e0, e1);
    };
    static_for<4>([&](auto jc) { p_word(std::integral_constant<int, 0>{}, jc); });
    __builtin_amdgcn_sched_barrier(0);
    // O^T += V^T . P^T
    static_for<4 * DB>([&](auto ic) {
      constexpr int i = decltype(ic)::value, g16 = i / DB, db = i % DB;
      const u32x4 f = vf[i % VR];
      if constexpr (i + VR < 4 * DB) vf[i % VR] = v_read(std::integral_constant<int, i + VR>{});
      o[db] = Mma32<T>::mfma(f, pb[g16], o[db]);
      if constexpr (g16 + 1 < 4) p_word(std::integral_constant<int, g16 + 1>{}, std::integral_constant<int, db>{});
      __builtin_amdgcn_sched_barrier(0);
    });
    l_run += psum;
  };

  // ---- pipeline: registers hold tile t + 1 while tile t is computed from LDS buffer t & 1; in interval t they are
  // written to the other buffer (last read for tile t - 1, before the barrier that ended interval t - 1) and the loads
  // of tile t + 2 are issued.  One barrier per tile.  ntiles is uniform over the workgroup.
  if (ntiles > 0) {
    issue_loads(0);
    write_tile(0);
    if (1 < ntiles) issue_loads(1);
    __syncthreads();
    // waves 4-7 (the second wave of every SIMD) stage at the top of the interval, waves 0-3 at the bottom: while one
    // wave of a SIMD writes LDS and computes addresses, its partner is in its MFMA sections
    const bool stage_first = wave >= NW / 2;
    auto stage = [&](int t) __attribute__((always_inline)) {
      if (t + 1 < ntiles) write_tile(t + 1);
      if (t + 2 < ntiles) issue_loads(t + 2);
    };
    auto tile_loop = [&](int t_begin, int t_end, auto mode_c) __attribute__((always_inline)) {
      constexpr int MODE = decltype(mode_c)::value;
      for (int t = t_begin; t < t_end; ++t) {
        if (stage_first) stage(t);
        if constexpr (MODE < 2) compute(t, std::integral_constant<bool, MODE == 1>{});
        if (!stage_first) stage(t);
        __syncthreads();
      }
    };
    // a wave's tiles come in three runs (one loop each: two compute copies behind a branch in one loop spill):
    // interior while 64 t + 63 <= w_lo, masked while 64 t <= w_hi, staging only above its rows
    const int n2 = (w_rows && w_hi >= 0) ? min(w_hi / BN + 1, ntiles) : 0;
    const int n1 = (w_rows && w_lo >= 0) ? min((w_lo + 1) / BN, n2) : 0;
    tile_loop(0, n1, std::integral_constant<int, 0>{});
    tile_loop(n1, n2, std::integral_constant<int, 1>{});
    tile_loop(n2, ntiles, std::integral_constant<int, 2>{});
  }

  // ---- O^T / l -> out, m + log l -> lse ------------------------------------------------------------------------------
  if (!rok) return;
  const float l = xsum(l_run);
  const float inv = l > 0.f ? 1.0f / l : 0.f;
  T* op = (T*)p.o + (int64_t)(tok0 + rtok) * p.o_st + (int64_t)head * p.o_sh + 4 * hi;
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      const u32x2 w = {Mma<T>::pack2(o[db][4 * rq] * inv, o[db][4 * rq + 1] * inv),
                       Mma<T>::pack2(o[db][4 * rq + 2] * inv, o[db][4 * rq + 3] * inv)};
      *reinterpret_cast<u32x2*>(op + 32 * db + 8 * rq) = w;
    }
  if (p.lse != nullptr && hi == 0)
    p.lse[(int64_t)head * p.lse_sh + tok0 + rtok] = l > 0.f ? (m_run + log2f(l)) * kLn2 : -INFINITY;
}

// ---- merge_attn_states: one thread per 16-byte vector (8 elements) of one (token, head) ----------------------------
struct MergeParams {
  void* out; float* out_lse;
  const void *p_out, *s_out;
  const float *p_lse, *s_lse;
  int64_t items, o_st, o_sh, p_st, p_sh, s_st, s_sh, lse_sh;
  int H, chunks;
};

template <typename T>
__global__ __launch_bounds__(256) void merge_attn_states_kernel(const MergeParams p) {
  const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (it >= p.items) return;
  const int c = (int)(it % p.chunks);
  const int64_t th = it / p.chunks;
  const int h = (int)(th % p.H);
  const int64_t t = th / p.H;
  float pl = p.p_lse[h * p.lse_sh + t], sl = p.s_lse[h * p.lse_sh + t];
  pl = pl == INFINITY ? -INFINITY : pl;   // FA2's empty row (triton_merge_attn_states.py:59-65)
  sl = sl == INFINITY ? -INFINITY : sl;
  const float mx = fmaxf(pl, sl);
  // both sides empty: 0 and -inf (the reference computes exp(-inf - -inf) = NaN, which a later merge would inherit)
  float ps = 0.f, ss = 0.f, ol = -INFINITY;
  if (mx != -INFINITY) {
    const float pe = expf(pl - mx), se = expf(sl - mx), sum = pe + se;
    ps = pe / sum;   // the scales first, then the products (:88-92)
    ss = se / sum;
    ol = logf(sum) + mx;
  }
  if (c == 0 && p.out_lse != nullptr) p.out_lse[h * p.lse_sh + t] = ol;
  const Vec<T, 8> pv = *reinterpret_cast<const Vec<T, 8>*>((const T*)p.p_out + t * p.p_st + h * p.p_sh + 8 * c);
  const Vec<T, 8> sv = *reinterpret_cast<const Vec<T, 8>*>((const T*)p.s_out + t * p.s_st + h * p.s_sh + 8 * c);
  Vec<T, 8> ov;
#pragma unroll
  for (int j = 0; j < 8; ++j) {   // an empty side contributes nothing, whatever its output holds
    const float a = ps == 0.f ? 0.f : to_f32(pv.v[j]) * ps;
    const float b = ss == 0.f ? 0.f : to_f32(sv.v[j]) * ss;
    ov.v[j] = from_f32<T>(a + b);
  }
  *reinterpret_cast<Vec<T, 8>*>((T*)p.out + t * p.o_st + h * p.o_sh + 8 * c) = ov;
}

static inline bool al16(const void* ptr) { return (((uintptr_t)ptr) & 15) == 0; }

}  // namespace mlap
}  // namespace va

extern "C" int vllm_amd_mla_prefill_attention(
    void* out, float* lse, const void* q, const void* k_nope, const void* k_pe, const void* v,
    const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, int batch, int64_t num_q_tokens, int num_heads,
    int qk_head_dim, int v_head_dim, int pe_dim, int max_seqlen_q, float sm_scale, int causal, int64_t q_stride_t,
    int64_t q_stride_h, int64_t o_stride_t, int64_t o_stride_h, int64_t kn_stride_t, int64_t kn_stride_h,
    int64_t kp_stride_t, int64_t kp_stride_h, int64_t v_stride_t, int64_t v_stride_h, int64_t lse_stride_h, int dtype,
    void* stream) {
  using namespace va;
  using namespace va::mlap;
  VA_REQUIRE(batch >= 0 && num_q_tokens >= 0 && num_heads > 0 && max_seqlen_q >= 0, VLLM_AMD_EINVAL,
             "mla_prefill_attention: bad shape");
  VA_REQUIRE(dtype == VLLM_AMD_BF16 || dtype == VLLM_AMD_F16, VLLM_AMD_EUNSUPPORTED,
             "mla_prefill_attention: q, k, v and out must be bfloat16 or float16");
  VA_REQUIRE(qk_head_dim == DN + DP && v_head_dim == DV && pe_dim == DP, VLLM_AMD_EUNSUPPORTED,
             "mla_prefill_attention: head dims q.k %d / v %d / rope %d; only 192 / 128 / 64 is implemented", qk_head_dim,
             v_head_dim, pe_dim);
  VA_REQUIRE(sm_scale > 0.f && sm_scale < INFINITY, VLLM_AMD_EINVAL, "mla_prefill_attention: sm_scale must be positive");
  if (batch == 0 || num_q_tokens == 0 || max_seqlen_q == 0) return VLLM_AMD_OK;
  VA_REQUIRE(out && q && k_nope && k_pe && v && cu_seqlens_q && cu_seqlens_k, VLLM_AMD_EINVAL,
             "mla_prefill_attention: null pointer");
  VA_REQUIRE(al16(out) && al16(q) && al16(k_nope) && al16(k_pe) && al16(v), VLLM_AMD_EINVAL,
             "mla_prefill_attention: q, k_nope, k_pe, v and out must be 16-byte aligned");
  VA_REQUIRE((q_stride_t | q_stride_h | o_stride_t | o_stride_h | kn_stride_t | kn_stride_h | kp_stride_t | kp_stride_h |
              v_stride_t | v_stride_h) % 8 == 0 &&
                 q_stride_t >= 0 && q_stride_h >= 0 && o_stride_t >= 0 && o_stride_h >= 0 && kn_stride_t >= 0 &&
                 kn_stride_h >= 0 && kp_stride_t >= 0 && kp_stride_h >= 0 && v_stride_t >= 0 && v_stride_h >= 0,
             VLLM_AMD_EINVAL, "mla_prefill_attention: token and head strides must be non-negative multiples of 8 elements");
  VA_REQUIRE(lse == nullptr || lse_stride_h >= num_q_tokens, VLLM_AMD_EINVAL,
             "mla_prefill_attention: lse head stride %lld < %lld tokens", (long long)lse_stride_h,
             (long long)num_q_tokens);
  const int64_t packed = num_q_tokens / BM + batch, even = (int64_t)batch * ceil_div(max_seqlen_q, BM);
  const int64_t gx = even <= packed ? even : packed;
  VA_REQUIRE(num_q_tokens < (1ll << 31) && gx * num_heads < (1ll << 31) && num_heads <= 65535, VLLM_AMD_EINVAL,
             "mla_prefill_attention: launch too large");
  Params p;
  p.o = out; p.lse = lse; p.q = q; p.k_nope = k_nope; p.k_pe = k_pe; p.v = v;
  p.cu_q = cu_seqlens_q; p.cu_k = cu_seqlens_k;
  p.num_seqs = batch; p.blocks_per_seq = even <= packed ? ceil_div(max_seqlen_q, BM) : 0; p.causal = causal != 0;
  p.sm_scale = sm_scale;
  p.q_st = q_stride_t; p.q_sh = q_stride_h; p.o_st = o_stride_t; p.o_sh = o_stride_h;
  p.kn_st = kn_stride_t; p.kn_sh = kn_stride_h; p.kp_st = kp_stride_t; p.kp_sh = kp_stride_h;
  p.v_st = v_stride_t; p.v_sh = v_stride_h; p.lse_sh = lse_stride_h;
  const dim3 grid((unsigned)gx, (unsigned)num_heads);
  if (dtype == VLLM_AMD_BF16)
    hipLaunchKernelGGL((mla_prefill_kernel<bf16_t>), grid, dim3(64 * NW), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL((mla_prefill_kernel<f16_t>), grid, dim3(64 * NW), 0, (hipStream_t)stream, p);
  VA_LAUNCH_CHECK("mla_prefill_attention launch");
  return VLLM_AMD_OK;
}

extern "C" int vllm_amd_merge_attn_states(void* out, float* out_lse, const void* prefix_out, const float* prefix_lse,
                                          const void* suffix_out, const float* suffix_lse, int64_t num_tokens,
                                          int num_heads, int head_size, int64_t out_stride_t, int64_t out_stride_h,
                                          int64_t prefix_stride_t, int64_t prefix_stride_h, int64_t suffix_stride_t,
                                          int64_t suffix_stride_h, int64_t lse_stride_h, int dtype, void* stream) {
  using namespace va;
  using namespace va::mlap;
  VA_REQUIRE(num_tokens >= 0 && num_heads > 0, VLLM_AMD_EINVAL, "merge_attn_states: bad shape");
  VA_REQUIRE(dtype == VLLM_AMD_BF16 || dtype == VLLM_AMD_F16, VLLM_AMD_EUNSUPPORTED,
             "merge_attn_states: outputs must be bfloat16 or float16");
  VA_REQUIRE(head_size > 0 && head_size <= 512 && head_size % 8 == 0, VLLM_AMD_EUNSUPPORTED,
             "merge_attn_states: head size %d is not a multiple of 8 up to 512", head_size);
  if (num_tokens == 0) return VLLM_AMD_OK;
  VA_REQUIRE(out && prefix_out && prefix_lse && suffix_out && suffix_lse, VLLM_AMD_EINVAL,
             "merge_attn_states: null pointer");
  VA_REQUIRE(al16(out) && al16(prefix_out) && al16(suffix_out) &&
                 (out_stride_t | out_stride_h | prefix_stride_t | prefix_stride_h | suffix_stride_t | suffix_stride_h) % 8 == 0 &&
                 out_stride_t >= 0 && out_stride_h >= 0 && prefix_stride_t >= 0 && prefix_stride_h >= 0 &&
                 suffix_stride_t >= 0 && suffix_stride_h >= 0,
             VLLM_AMD_EINVAL, "merge_attn_states: outputs must be 16-byte aligned with strides that are multiples of 8 elements");
  VA_REQUIRE(lse_stride_h >= num_tokens, VLLM_AMD_EINVAL, "merge_attn_states: lse head stride %lld < %lld tokens",
             (long long)lse_stride_h, (long long)num_tokens);
  MergeParams p;
  p.out = out; p.out_lse = out_lse; p.p_out = prefix_out; p.s_out = suffix_out; p.p_lse = prefix_lse; p.s_lse = suffix_lse;
  p.H = num_heads; p.chunks = head_size / 8;
  p.items = num_tokens * num_heads * p.chunks;
  p.o_st = out_stride_t; p.o_sh = out_stride_h; p.p_st = prefix_stride_t; p.p_sh = prefix_stride_h;
  p.s_st = suffix_stride_t; p.s_sh = suffix_stride_h; p.lse_sh = lse_stride_h;
  const int64_t blocks = (p.items + 255) / 256;
  VA_REQUIRE(blocks < (1ll << 31), VLLM_AMD_EINVAL, "merge_attn_states: launch too large");
  if (dtype == VLLM_AMD_BF16)
    hipLaunchKernelGGL((merge_attn_states_kernel<bf16_t>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL((merge_attn_states_kernel<f16_t>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
  VA_LAUNCH_CHECK("merge_attn_states launch");
  return VLLM_AMD_OK;
}
