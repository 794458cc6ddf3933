// Multi-head latent attention (MLA) decode over the latent KV cache, for gfx950.
//
//   cache  [num_blocks, page_size, 576]   one row per token: 512 latent columns (kv_c), then 64
//                                         rotary columns (k_pe); shared by every query head
//   q      [B, H, 576]                    o [B, H, 512]
//   logits = sm_scale * q . row (all 576 columns), softmax over the sequence's tokens, o = sum p * row[0:512]
//
// Semantics: _fwd_grouped_kernel_stage1 + _fwd_kernel_stage2 of the reference's
// vllm/attention/ops/triton_decode_attention.py:228-378, 471-525 as the MLA backend calls them
// (vllm/v1/attention/backends/mla/triton_mla.py:124-171): fp32 online softmax, the probabilities rounded
// to the data type before PV (their sum is taken before the rounding, as there), split s of a sequence
// covers tokens [s L, min((s + 1) L, len)) with L = ceil(len / num_kv_splits), empty splits write and
// read nothing, partials are merged by log-sum-exp.  DEVIATION: a sequence of length 0 gets a ZERO output
// row; the reference computes 0 / 0 there.  logit_cap is not supported (the reference's MLA backend rejects
// it, triton_mla.py:55-59).  An fp8 (e4m3) cache, which that backend also rejects (:134-135), is served
// too (vllm_amd_mla_decode_fp8, with the cache's scale).
//
// ONE kernel, mla_decode_kernel<T, Fmt, G>, serves both cache formats.  The skeleton below (grid, row
// loads, ring, waits, softmax bookkeeping, epilogue) is written once; Fmt (MlaRows16<T>: a cache of T,
// MlaRowsFp8<T>: a cache of e4m3fn bytes) holds the tile size, the LDS row and the three pieces of math
// that depend on them: the QK product of one item, the P write, the PV product, plus the orders of the q
// fragments and of the output columns that follow from those.
//
// Work split.  One workgroup (8 waves) = one (sequence, split, chunk of 16 G heads), G = 1 or 2
// ("heads per workgroup" 16 / 32, chosen by the launcher, tuning key "mla_hpw").  G = 4 is written (the
// template covers it) but not instantiated: as compiled for the 16-bit cache it needs about 270 of the
// 256 registers a wave of an 8-wave workgroup has and spills four q fragments.  The workgroup walks its
// tokens in tiles of T = Fmt::TOK:
//   * rows -> LDS: global_load_lds, 16 B per lane, straight from the paged cache (gather granularity =
//     one token, any page size) into a ring of 3 stages, two tiles in flight under the current tile's
//     math.  A row is fetched ONCE per workgroup and serves both products from LDS.  The LDS image pads a
//     row by one chunk of 16 B (Fmt::CH chunks) so that the operand reads are conflict-free (per format,
//     below); either format's tile fits 5 LDS-DMA per lane and 40 960 B per stage.
//   * S = K q^T: mfma_f32_16x16x32 of the q type, A = 16 token rows x 32 columns, B = q (16 heads), 18
//     steps over the 576 columns.  The (T / 16) G (token subtile, head group) items go to waves
//     0 .. (T / 16) G - 1 (wave gq + G sub holds subtile sub of group gq); a wave keeps the q fragments of
//     its group in 72 registers for the whole split.  Result: lane (c16, g4) holds tokens 4 g4 .. + 3 of
//     head c16.
//   * softmax: per-wave row maxima and sums meet in LDS (two barriers per tile); every wave tracks the
//     running maximum and sum of all 16 G heads (lane c16 <-> head c16 of each group), so no wave waits
//     for another one's rescale factor.  P is rounded to the data type and written to LDS, never
//     quantised.
//   * O^T += V^T P^T: the 16 x 512 output of a head group is divided by V column: wave w owns columns
//     [64 w, 64 w + 64) of ALL G groups (16 G accumulator registers).  A = V^T: lane (c16, g4) needs
//     one column of 8 tokens per 32, i.e. the token index is the contraction index -- a transposing read
//     by hand, whose slot order is also the order P is stored in ([head][g4][i], rows of 80 B), so that
//     a P fragment is one ds_read_b128.  Each V fragment is used by G MFMAs.
//   * every LDS access of the loop is inline assembly: hipcc orders a C++ LDS access behind ALL
//     outstanding LDS-DMA, which would drain the ring every tile.  The waits are: lgkmcnt(0) inside each
//     read block / in front of each barrier, and one counted vmcnt in front of the tile's first barrier.
//     Per tile a lane issues 5 block-table loads (for tile t + 3) and THEN its 5 LDS-DMA (tile t + 2),
//     so "at most 5 outstanding" = only the youngest tile's DMA is still in flight = tile t has landed.
//     The block-table entries are loaded one tile before their DMA so that their use does not wait for
//     the younger DMA in front of them (as compiled, the compiler's own wait at two of those uses per
//     pair of tiles is still vmcnt(0): DESIGN.md, open items).
//   * num_kv_splits == 1 writes o directly; otherwise the normalised partial row and the split's
//     log-sum-exp go to the caller's attn_logits ([B, H, splits, 512] rows, then [B, H, splits] lse: the
//     tensor's 513 floats per split, regrouped so that rows stay 16-byte aligned) and mla_merge_kernel
//     combines the non-empty splits.
// H = 128 runs as four chunks of 32 heads: the later chunks' rows are meant to come from L2 (chunks of
// one (sequence, split) sit next to each other on the same XCD), so that HBM sees each row once per
// (sequence, split).
//
// The 16-bit cache (MlaRows16), T = 32:
//   * A row is 73 chunks in LDS (1168 B = 292 words, 36 mod 64 banks): 16 consecutive rows then start in
//     16 different 4-bank groups, which makes the K-operand reads (16 rows x 16 B per pass) conflict-free,
//     and rows r .. r + 3 are 36 words apart, which does the same for the V-operand reads.
//   * S: a K fragment is one ds_read_b128 per lane, 18 per item; q fragment j is columns 32 j + 8 g4 .. + 7.
//   * PV: a V^T fragment is 8 ds_read_u16 (+ 4 shift-or): contraction slot (g4, i) is token 4 i + g4, so
//     one read instruction touches rows i*4 .. i*4 + 3 (36 words apart) x 16 consecutive 16-bit columns
//     (8 words): 32 distinct banks.  Column tile ct of a wave is columns 64 w + 16 ct + 4 m (m = MFMA row).
//   * P is written as 4 ds_write_b16 (token 16 sub + 4 g4 + r = slot (r, 4 sub + g4)).
//
// The fp8 cache (MlaRowsFp8): [num_blocks, page_size, 576] BYTES, value = float(byte) * kv_scale (what
// concat_and_cache_mla writes for kv_cache_dtype "fp8").  The tiling is its own, because a row is half as
// big:
//   * T = 64.  A row is staged as bytes, padded to 37 chunks (592 B = 148 words, 20 mod 64 banks): 64 x 37
//     = 2368 chunks fit the same 5 LDS-DMA per lane and stage.  One barrier chain (wait, S, softmax, PV)
//     covers 64 tokens.
//   * The operands are widened in registers when a fragment is read (v_cvt_scalef32_pk_{bf16,f16}_fp8,
//     scale 1: exact), q is never quantised.  kv_scale never touches an operand: it is folded into the
//     logit scale and into the epilogue's 1 / l.
//   * S: a lane reads 16 bytes of its token row (ds_read_b128) and widens them into TWO A fragments, so
//     contraction step (jj, half) is columns 64 jj + 16 g4 + 8 half .. + 7; the resident q fragments are
//     loaded in that order.  9 reads, 72 conversions, 18 MFMAs per item.  With G = 2 every wave has one.
//   * PV: column tile ct holds the columns 64 w + 4 m + ct (m = MFMA row), so that ONE ds_read_b32 per
//     token gives a lane its byte of all four column tiles: the byte gather is 8 reads per 32 tokens (16
//     per tile) instead of 8 per fragment.  Contraction slot (g4, i) of step ks is token 32 ks + 16 (i / 4)
//     + 4 g4 + i % 4; four v_perm_b32 pair the bytes of two tokens, and the conversions take the pairs
//     apart by column.  A lane ends up with the 16 consecutive columns 64 w + 16 g4 + 4 r + ct.
//   * P is written as 8 bytes (tokens 4 g4 .. + 3 of a subtile are consecutive slots) into [step][group]
//     [head] rows of 80 B and read back as one ds_read_b128 per step and group.
//   * Bank conflicts, checked by enumerating bank = (byte address / 4) % 64 over the lanes of one access
//     pass: K reads, 16 lanes (rows c16, 4 words each): row starts 20 c16 mod 64 = {0, 20, 40, 60, 16, 36,
//     56, 12, 32, 52, 8, 28, 48, 4, 24, 44}, sixteen disjoint 4-bank groups.  V reads, 64 lanes: rows
//     4 g4 + const start 80 g4 = 16 g4 (mod 64) words apart, each with the 16 consecutive words of c16: 64
//     distinct banks.  P reads: rows of 20 words, as the K reads.  The P write (8 bytes per lane, once per
//     tile) has two-way conflicts between a row's second half and another row's first; it was left alone.
//     Not measured on the device (no counter run).
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): see DESIGN.md.
// Nothing is allocated or synchronised and there is no workspace beyond attn_logits: graph-capturable.
#include "mma.cuh"

namespace va {

typedef __attribute__((ext_vector_type(4))) int i32x4;

constexpr int MLA_DK = 576, MLA_DV = 512;
constexpr int MLA_NW = 8, MLA_NT = MLA_NW * 64;     // waves, threads
constexpr int MLA_PER = 5;                          // LDS-DMA per lane and stage: 5 * 512 >= 32 * 73, 64 * 37
constexpr int MLA_STAGE = MLA_PER * MLA_NT * 16;    // 40960
constexpr int MLA_NST = 3;
constexpr int MLA_PROW = 80, MLA_PGRP = 16 * MLA_PROW;   // P: [slab][head][32 slots], rows padded to 80 B
// the 16-bit cache
constexpr int MLA_T = 32;                           // tokens per tile
constexpr int MLA_CH = 73;                          // 16-byte chunks per LDS row (72 + 1 pad)
constexpr int MLA_ROWB = MLA_CH * 16;               // 1168
// the fp8 cache
constexpr int M8_T = 64;                            // tokens per tile
constexpr int M8_CH = 37;                           // 16-byte chunks per LDS row (36 + 1 pad)
constexpr int M8_ROWB = M8_CH * 16;                 // 592

int g_mla_hpw = 0;   // tuning "mla_hpw": 0 = by H, 16 / 32 = heads per workgroup

// ---- LDS access of the main loop (see the header) -------------------------------------------------
template <int OFF>
__device__ __forceinline__ void lds_read3(uint32_t addr, i32x4 (&v)[3]) {
  asm volatile(
      "ds_read_b128 %0, %3 offset:%4\n\tds_read_b128 %1, %3 offset:%5\n\tds_read_b128 %2, %3 offset:%6\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2])
      : "v"(addr), "n"(OFF), "n"(OFF + 64), "n"(OFF + 128)
      : "memory");
}
// N floats, 64 bytes apart
template <int N>
__device__ __forceinline__ void lds_read_f32(uint32_t addr, float (&v)[N]) {
  static_assert(N == 2 || N == 4 || N == 8, "");
  if constexpr (N == 2) {
    asm volatile("ds_read_b32 %0, %2\n\tds_read_b32 %1, %2 offset:64\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(v[0]), "=&v"(v[1]) : "v"(addr) : "memory");
  } else if constexpr (N == 4) {
    asm volatile("ds_read_b32 %0, %4\n\tds_read_b32 %1, %4 offset:64\n\tds_read_b32 %2, %4 offset:128\n\t"
                 "ds_read_b32 %3, %4 offset:192\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]) : "v"(addr) : "memory");
  } else {
    asm volatile("ds_read_b32 %0, %8\n\tds_read_b32 %1, %8 offset:64\n\tds_read_b32 %2, %8 offset:128\n\t"
                 "ds_read_b32 %3, %8 offset:192\n\tds_read_b32 %4, %8 offset:256\n\tds_read_b32 %5, %8 offset:320\n\t"
                 "ds_read_b32 %6, %8 offset:384\n\tds_read_b32 %7, %8 offset:448\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]),
                   "=&v"(v[7])
                 : "v"(addr) : "memory");
  }
}
// the 16-bit V^T fragment of 16 columns: the elements (row 4 i + g4, column c16), i = 0 .. 7; the lane's
// address already holds g4 and c16, OFF the column tile.  Eight zero-extending 16-bit reads, paired by
// four shift-or instructions (the d16 forms that would write register halves directly do not keep the
// other half on this chip: with SRAM ECC they clear it).
template <int OFF>
__device__ __forceinline__ i32x4 lds_read_vt(uint32_t addr) {
  constexpr int R4 = 4 * MLA_ROWB;
  uint32_t e[8];
  asm volatile(
      "ds_read_u16 %0, %8 offset:%9\n\tds_read_u16 %1, %8 offset:%10\n\t"
      "ds_read_u16 %2, %8 offset:%11\n\tds_read_u16 %3, %8 offset:%12\n\t"
      "ds_read_u16 %4, %8 offset:%13\n\tds_read_u16 %5, %8 offset:%14\n\t"
      "ds_read_u16 %6, %8 offset:%15\n\tds_read_u16 %7, %8 offset:%16\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(e[0]), "=&v"(e[1]), "=&v"(e[2]), "=&v"(e[3]), "=&v"(e[4]), "=&v"(e[5]), "=&v"(e[6]), "=&v"(e[7])
      : "v"(addr), "n"(OFF), "n"(OFF + R4), "n"(OFF + 2 * R4), "n"(OFF + 3 * R4), "n"(OFF + 4 * R4),
        "n"(OFF + 5 * R4), "n"(OFF + 6 * R4), "n"(OFF + 7 * R4)
      : "memory");
  return (i32x4){(int)(e[0] | e[1] << 16), (int)(e[2] | e[3] << 16), (int)(e[4] | e[5] << 16),
                 (int)(e[6] | e[7] << 16)};
}
// the fp8 bytes (token slot i = 0 .. 7 of step OFF, columns 4 c16 .. + 3 of the wave's 64): rows i % 4 and
// 16 + i % 4 past the lane's own (which holds 4 g4)
template <int OFF>
__device__ __forceinline__ void lds_read_v8(uint32_t addr, uint32_t (&w)[8]) {
  constexpr int R = M8_ROWB;
  asm volatile(
      "ds_read_b32 %0, %8 offset:%9\n\tds_read_b32 %1, %8 offset:%10\n\t"
      "ds_read_b32 %2, %8 offset:%11\n\tds_read_b32 %3, %8 offset:%12\n\t"
      "ds_read_b32 %4, %8 offset:%13\n\tds_read_b32 %5, %8 offset:%14\n\t"
      "ds_read_b32 %6, %8 offset:%15\n\tds_read_b32 %7, %8 offset:%16\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(w[0]), "=&v"(w[1]), "=&v"(w[2]), "=&v"(w[3]), "=&v"(w[4]), "=&v"(w[5]), "=&v"(w[6]), "=&v"(w[7])
      : "v"(addr), "n"(OFF), "n"(OFF + R), "n"(OFF + 2 * R), "n"(OFF + 3 * R), "n"(OFF + 16 * R),
        "n"(OFF + 17 * R), "n"(OFF + 18 * R), "n"(OFF + 19 * R)
      : "memory");
}
// the P^T fragments of G head groups, MLA_PGRP bytes apart
template <int G>
__device__ __forceinline__ void lds_read_p(uint32_t addr, i32x4 (&v)[G]) {
  static_assert(G == 1 || G == 2 || G == 4, "");
  if constexpr (G == 1) {
    asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(v[0]) : "v"(addr) : "memory");
  } else if constexpr (G == 2) {
    asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:%3\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(v[0]), "=&v"(v[1]) : "v"(addr), "n"(MLA_PGRP) : "memory");
  } else {
    asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:%5\n\tds_read_b128 %2, %4 offset:%6\n\t"
                 "ds_read_b128 %3, %4 offset:%7\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3])
                 : "v"(addr), "n"(MLA_PGRP), "n"(2 * MLA_PGRP), "n"(3 * MLA_PGRP) : "memory");
  }
}
__device__ __forceinline__ void lds_write_b32(uint32_t addr, float v) {
  asm volatile("ds_write_b32 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
template <int OFF>
__device__ __forceinline__ void lds_write_b16(uint32_t addr, uint32_t v) {
  asm volatile("ds_write_b16 %0, %1 offset:%2" ::"v"(addr), "v"(v), "n"(OFF) : "memory");
}
__device__ __forceinline__ void lds_write_b64(uint32_t addr, uint64_t v) {
  asm volatile("ds_write_b64 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
__device__ __forceinline__ void lds_barrier() {   // own LDS traffic done, then everybody's
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

template <typename T> __device__ __forceinline__ uint32_t bits16(T v) {
  return (uint32_t)__builtin_bit_cast(uint16_t, v);
}

// ---------------------------------------------------------------------------------------------
// the two cache formats: what the kernel below asks of a format (see the header for the layouts).
// Lane (c16, g4) of wave `wave`; QK item = (head group gq, token subtile sub); LDS addresses are
// relative to the stage (k, v) or to the P area (p).
// ---------------------------------------------------------------------------------------------
template <typename T>
struct MlaRows16 {
  typedef T elem;                                      // cache element, EPC of them in a 16-byte chunk
  static constexpr int TOK = MLA_T, CH = MLA_CH, ROWB = MLA_ROWB, EPC = 8;

  // the kernel's float pointers: the splits' scratch; a cache element is its value, so there is no scale
  // and no kernel argument for one (see the kernel)
  typedef float* __restrict__ Floats;
  static Floats floats(float* scratch, const float*) { return scratch; }
  static __device__ __forceinline__ float* scratch_of(Floats f) { return f; }
  static __device__ __forceinline__ float cache_scale(Floats) { return 1.0f; }
  // first q column of fragment j
  static __device__ __forceinline__ int q_col(int j, int g4) { return 32 * j + 8 * g4; }
  static __device__ __forceinline__ uint32_t v_off(int wave, int c16, int g4) {
    return g4 * ROWB + (64 * wave + c16) * 2;
  }
  template <int G>
  static __device__ __forceinline__ uint32_t p_off(int gq, int sub, int c16, int g4) {
    return gq * MLA_PGRP + c16 * MLA_PROW + (4 * sub + g4) * 2;
  }

  // s0 + s1 = K q^T of the item whose 16 rows start at k_lds
  static __device__ __forceinline__ void qk(uint32_t k_lds, const i32x4 (&qf)[18], f32x4& s0, f32x4& s1) {
    static_for<6>([&](auto jc) {
      constexpr int j0 = decltype(jc)::value * 3;
      i32x4 kf[3];
      lds_read3<j0 * 64>(k_lds, kf);
      s0 = Mma<T>::mfma(__builtin_bit_cast(uint4, kf[0]), __builtin_bit_cast(uint4, qf[j0]), s0);
      s1 = Mma<T>::mfma(__builtin_bit_cast(uint4, kf[1]), __builtin_bit_cast(uint4, qf[j0 + 1]), s1);
      s0 = Mma<T>::mfma(__builtin_bit_cast(uint4, kf[2]), __builtin_bit_cast(uint4, qf[j0 + 2]), s0);
    });
  }
  // token 16 sub + 4 g4 + r = contraction slot (r, 4 sub + g4)
  static __device__ __forceinline__ void p_write(uint32_t p_lds, const uint32_t (&pb)[4]) {
    lds_write_b16<0>(p_lds, pb[0]);
    lds_write_b16<16>(p_lds, pb[1]);
    lds_write_b16<32>(p_lds, pb[2]);
    lds_write_b16<48>(p_lds, pb[3]);
  }
  template <int G>
  static __device__ __forceinline__ void pv(uint32_t p_lds, uint32_t v_lds, f32x4 (&acc)[G][4]) {
    i32x4 pf[G];
    lds_read_p<G>(p_lds, pf);
    static_for<4>([&](auto cc) {
      constexpr int ct = decltype(cc)::value;
      const i32x4 vf = lds_read_vt<ct * 32>(v_lds);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        acc[g][ct] = Mma<T>::mfma(__builtin_bit_cast(uint4, vf), __builtin_bit_cast(uint4, pf[g]), acc[g][ct]);
      }
    });
  }
  // the lane's i-th run of 4 consecutive output columns: acc[ct][r] is column 64 wave + 16 ct + 4 g4 + r
  static __device__ __forceinline__ f32x4 out4(const f32x4 (&acc)[4], int i, int wave, int g4, int& col) {
    col = 64 * wave + 16 * i + 4 * g4;
    return acc[i];
  }
};

template <typename T>
struct MlaRowsFp8 {
  typedef uint8_t elem;
  static constexpr int TOK = M8_T, CH = M8_CH, ROWB = M8_ROWB, EPC = 16;

  struct Floats {   // the splits' scratch and the cache's scale, a device float[1]
    float* scratch;
    const float* kv_scale;
  };
  static Floats floats(float* scratch, const float* kv_scale) { return {scratch, kv_scale}; }
  static __device__ __forceinline__ float* scratch_of(const Floats& f) { return f.scratch; }
  static __device__ __forceinline__ float cache_scale(const Floats& f) { return f.kv_scale[0]; }
  // in the order the widened K fragments come: fragment 2 jj + half = columns 64 jj + 16 g4 + 8 half .. + 7
  static __device__ __forceinline__ int q_col(int j, int g4) { return 64 * (j >> 1) + 16 * g4 + 8 * (j & 1); }
  static __device__ __forceinline__ uint32_t v_off(int wave, int c16, int g4) {
    return 4 * g4 * ROWB + 64 * wave + 4 * c16;
  }
  template <int G>
  static __device__ __forceinline__ uint32_t p_off(int gq, int sub, int c16, int g4) {
    return ((sub >> 1) * G + gq) * MLA_PGRP + c16 * MLA_PROW + g4 * 16 + (sub & 1) * 8;
  }

  static __device__ __forceinline__ void qk(uint32_t k_lds, const i32x4 (&qf)[18], f32x4& s0, f32x4& s1) {
    static_for<3>([&](auto jc) {
      constexpr int j0 = decltype(jc)::value * 3;
      i32x4 kf[3];
      lds_read3<j0 * 64>(k_lds, kf);
      static_for<3>([&](auto ic) {
        constexpr int jj = j0 + decltype(ic)::value;
        uint4 lo, hi;
        widen16<T>(__builtin_bit_cast(uint4, kf[decltype(ic)::value]), lo, hi);
        s0 = Mma<T>::mfma(lo, __builtin_bit_cast(uint4, qf[2 * jj]), s0);
        s1 = Mma<T>::mfma(hi, __builtin_bit_cast(uint4, qf[2 * jj + 1]), s1);
      });
    });
  }
  // token 16 sub + 4 g4 + r = slot (g4, 4 (sub % 2) + r) of step sub / 2
  static __device__ __forceinline__ void p_write(uint32_t p_lds, const uint32_t (&pb)[4]) {
    lds_write_b64(p_lds, (uint64_t)(pb[0] | pb[1] << 16) | (uint64_t)(pb[2] | pb[3] << 16) << 32);
  }
  template <int G>
  static __device__ __forceinline__ void pv(uint32_t p_lds, uint32_t v_lds, f32x4 (&acc)[G][4]) {
    static_for<2>([&](auto kc) {
      constexpr int ks = decltype(kc)::value;
      i32x4 pf[G];
      lds_read_p<G>(p_lds + ks * G * MLA_PGRP, pf);
      uint32_t w[8], pr[2][4];
      lds_read_v8<ks * 32 * M8_ROWB>(v_lds, w);
      // bytes of tokens (2 p, 2 p + 1): pr[0][p] = columns 0, 0, 1, 1; pr[1][p] = columns 2, 2, 3, 3
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        pr[0][p] = __builtin_amdgcn_perm(w[2 * p + 1], w[2 * p], 0x05010400u);
        pr[1][p] = __builtin_amdgcn_perm(w[2 * p + 1], w[2 * p], 0x07030602u);
      }
      static_for<4>([&](auto cc) {
        constexpr int ct = decltype(cc)::value;
        uint4 vf;
        vf.x = Mma<T>::cvt2(pr[ct >> 1][0], ct & 1);
        vf.y = Mma<T>::cvt2(pr[ct >> 1][1], ct & 1);
        vf.z = Mma<T>::cvt2(pr[ct >> 1][2], ct & 1);
        vf.w = Mma<T>::cvt2(pr[ct >> 1][3], ct & 1);
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g][ct] = Mma<T>::mfma(vf, __builtin_bit_cast(uint4, pf[g]), acc[g][ct]);
      });
    });
  }
  // acc[ct][r] is column 64 wave + 16 g4 + 4 r + ct
  static __device__ __forceinline__ f32x4 out4(const f32x4 (&acc)[4], int i, int wave, int g4, int& col) {
    col = 64 * wave + 16 * g4 + 4 * i;
    return (f32x4){acc[0][i], acc[1][i], acc[2][i], acc[3][i]};
  }
};

// ---------------------------------------------------------------------------------------------
// main kernel.  fl = Fmt::Floats, the splits' scratch and, where the format has one, the cache's scale: a
// format without a scale has no argument for it, because an unused pointer argument (in front of or behind
// the others) moves the kernel-argument loads and with them the compiler's schedule outside the tile loop,
// which measured as about 1 % on the 32-head variants.
// ---------------------------------------------------------------------------------------------
template <typename T, typename Fmt, int G>
__global__ __launch_bounds__(MLA_NT) void mla_decode_kernel(
    T* __restrict__ o, const T* __restrict__ q, const typename Fmt::elem* __restrict__ cache,
    const int* __restrict__ block_table, const int* __restrict__ seq_lens, typename Fmt::Floats fl, int B, int H,
    int S, int NC, int page_size, uint32_t ps_magic, int max_blocks, float sm_log2e, int64_t q_sb, int64_t q_sh,
    int64_t o_sb, int64_t o_sh, int64_t c_sb, int64_t c_se, int64_t bt_s, int o_vec) {
  constexpr int TOK = Fmt::TOK;
  constexpr int NSUB = TOK / 16;    // QK token subtiles (one MFMA's rows) per head group
  constexpr int NQ = NSUB * G;      // waves with a QK item
  constexpr int NPS = TOK / 32 * G;   // P slabs: one per PV contraction step (32 tokens) and group
  constexpr int P_OFF = MLA_NST * MLA_STAGE, MAX_OFF = P_OFF + NPS * MLA_PGRP, SUM_OFF = MAX_OFF + MLA_NW * 64;
  static_assert(MLA_PER * MLA_NT >= TOK * Fmt::CH, "a stage holds a tile");
  static_assert(NSUB % 2 == 0 && (NSUB & (NSUB - 1)) == 0 && TOK <= 256, "subtiles pair up; a row fits 8 bits");
  static_assert(NQ <= MLA_NW && SUM_OFF + MLA_NW * 64 <= 160 * 1024, "waves, LDS");
  __shared__ __attribute__((aligned(16))) uint8_t lds[SUM_OFF + MLA_NW * 64];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c16 = lane & 15, g4 = lane >> 4;

  // hardware workgroup i runs on XCD i % 8: the NC head chunks of one (sequence, split) take
  // consecutive slots of ONE XCD, so all but the first find the rows in that XCD's L2
  const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
  const int chunk = idx % NC, u = (idx / NC) * 8 + xcd;
  if (u >= B * S) return;
  const int b = u / S, split = u - b * S;
  const int h0 = chunk * 16 * G;
  const int len = seq_lens[b];
  if (len <= 0) {
    if (S == 1)   // the merge kernel writes the zero row otherwise
      for (int i = tid; i < 16 * G * MLA_DV; i += MLA_NT) {
        const int h = h0 + i / MLA_DV;
        if (h < H) o[b * o_sb + h * o_sh + i % MLA_DV] = from_f32<T>(0.f);
      }
    return;
  }
  const int L = (len + S - 1) / S;
  const int start = split * L, end = min(start + L, len);
  if (start >= end) return;
  const int ntiles = (end - start + TOK - 1) / TOK;
  const float kvs = Fmt::cache_scale(fl);
  const float scale2 = sm_log2e * kvs;

  const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)lds;

  // ---- the row-load path (the one place a converting load would go): LDS position p = 512 r + tid of
  // a stage is chunk p % CH of tile row p / CH; pad chunks and positions past the tile re-read chunk 0
  // (never used).  Rows past the split's end re-read its last token: finite data under a zero weight.
  int ppos[MLA_PER];   // row | first element << 8
#pragma unroll
  for (int r = 0; r < MLA_PER; ++r) {
    const int p = r * MLA_NT + tid;
    int row = p / Fmt::CH, c = p - row * Fmt::CH;
    if (row >= TOK) row = 0, c = 0;
    if (c == Fmt::CH - 1) c = 0;
    ppos[r] = row | (c * Fmt::EPC) << 8;
  }
  const int* bt_row = block_table + b * bt_s;
  // (the position passes through an empty asm: the 64-bit address parts derived from it would otherwise be
  // hoisted out of the tile loop, ten registers the 64-head variant does not have)
  auto locate = [&](int t, int r, int& pos, int& blk, int& within) {
    pos = ppos[r];
    asm volatile("" : "+v"(pos));
    const int tok = min(start + t * TOK + (pos & 255), end - 1);
    // tok / page_size without a branch: ps_magic = floor(2^32 / page_size) (2^32 - 1 for 1) gives the
    // quotient or one less
    blk = (int)__umulhi((uint32_t)tok, ps_magic);
    within = tok - blk * page_size;
    const bool fix = within >= page_size;
    blk += fix ? 1 : 0;
    within -= fix ? page_size : 0;
  };
  auto table_load = [&](int t, int (&page)[MLA_PER]) {
#pragma unroll
    for (int r = 0; r < MLA_PER; ++r) {
      int pos, blk, within;
      locate(t, r, pos, blk, within);
      page[r] = bt_row[min(blk, max_blocks - 1)];
    }
  };
  auto stage_rows = [&](int t, int stage, const int (&page)[MLA_PER]) {
    uint8_t* dst = lds + stage * MLA_STAGE + wave * 1024;
#pragma unroll
    for (int r = 0; r < MLA_PER; ++r) {
      int pos, blk, within;
      locate(t, r, pos, blk, within);
      const typename Fmt::elem* src = cache + (int64_t)page[r] * c_sb + (int64_t)within * c_se + (pos >> 8);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)(dst + r * MLA_NT * 16), 16, 0, 0);
    }
  };

  // ---- q fragments of this wave's QK item (group gq, token subtile sub), resident for the split
  const bool qk_wave = wave < NQ;
  const int gq = wave % G, sub = (wave / G) & (NSUB - 1);
  i32x4 qf[18];
  {
    const int head = h0 + gq * 16 + c16;
    const bool ok = qk_wave && head < H;
    const T* qrow = q + b * q_sb + (ok ? head : 0) * q_sh;
#pragma unroll
    for (int j = 0; j < 18; ++j) {
      qf[j] = *reinterpret_cast<const i32x4*>(qrow + Fmt::q_col(j, g4));
      if (!ok) qf[j] = (i32x4){0, 0, 0, 0};
    }
  }

  f32x4 acc[G][4];    // [group][column tile]: Fmt::out4 maps a register to its column of head c16
  float m[G], l[G];   // running maximum (log2 domain) and sum of head c16 of every group
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = -INFINITY;
    l[g] = 0.f;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[g][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }

  const uint32_t k_addr = lds_base + (16 * sub + c16) * Fmt::ROWB + g4 * 16;
  const uint32_t v_addr = lds_base + Fmt::v_off(wave, c16, g4);
  const uint32_t pw_addr = lds_base + P_OFF + Fmt::template p_off<G>(gq, sub, c16, g4);
  const uint32_t pr_addr = lds_base + P_OFF + c16 * MLA_PROW + g4 * 16;
  const uint32_t max_addr = lds_base + MAX_OFF + c16 * 4, sum_addr = lds_base + SUM_OFF + c16 * 4;

  int pgA[MLA_PER], pgB[MLA_PER];
  table_load(0, pgA);
  stage_rows(0, 0, pgA);
  asm volatile("" ::: "memory");
  table_load(1, pgB);
  table_load(2, pgA);
  asm volatile("" ::: "memory");
  stage_rows(1, 1, pgB);

  // one tile: `cur` holds the table entries of tile t + 2, `nxt` receives those of tile t + 3
  auto step = [&](int t, int stage, int (&cur_pg)[MLA_PER], int (&nxt_pg)[MLA_PER]) {
    // tile t has landed: since the previous tile's wait this lane issued the table loads of tile t + 2
    // and then the 5 DMA of tile t + 1; everything but those 5 youngest operations is complete (a
    // different issue order would only make this wait longer).  Tiles past the split's end are staged
    // like any other (they re-read the last token's row into a stage nobody reads): the loop has no
    // branch around its loads, which keeps the compiler's own wait counts exact.
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(MLA_PER) : "memory");
    lds_barrier();   // everybody's part of tile t has landed; everybody is past tile t - 1
    table_load(t + 3, nxt_pg);
    asm volatile("" ::: "memory");   // table loads first, DMA last
    stage_rows(t + 2, stage >= 1 ? stage - 1 : MLA_NST - 1, cur_pg);   // (t + 2) % 3

    const uint32_t so = stage * MLA_STAGE;
    const int nv = min(TOK, end - start - t * TOK);   // valid tokens of the tile

    // ---- S = K q^T for this wave's item
    float sv[4];
    if (qk_wave) {
      f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
      Fmt::qk(k_addr + so, qf, s0, s1);
      float lmax = -INFINITY;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        sv[r] = 16 * sub + 4 * g4 + r < nv ? (s0[r] + s1[r]) * scale2 : -INFINITY;
        lmax = fmaxf(lmax, sv[r]);
      }
      lmax = fmaxf(lmax, __shfl_xor(lmax, 16, 64));
      lmax = fmaxf(lmax, __shfl_xor(lmax, 32, 64));
      if (g4 == 0) lds_write_b32(max_addr + wave * 64, lmax);
    }
    lds_barrier();

    // ---- new maxima of all groups; every tile holds a valid token, so they are finite
    // (the accumulators and sums are rescaled here, so that the factors are dead before the PV phase)
    {
      float wm[NQ];
      lds_read_f32<NQ>(max_addr, wm);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float mn = m[g];
#pragma unroll
        for (int s = 0; s < NSUB; s += 2) mn = fmaxf(mn, fmaxf(wm[g + s * G], wm[g + (s + 1) * G]));
        const float alpha = fast_exp2(m[g] - mn);
        m[g] = mn;
        l[g] *= alpha;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[g][ct] *= alpha;
      }
    }
    if (qk_wave) {
      float mq = m[0];
#pragma unroll
      for (int g = 1; g < G; ++g) mq = gq == g ? m[g] : mq;
      float psum = 0.f;
      uint32_t pb[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = fast_exp2(sv[r] - mq);
        psum += p;
        pb[r] = bits16(from_f32<T>(p));
      }
      psum += __shfl_xor(psum, 16, 64);
      psum += __shfl_xor(psum, 32, 64);
      if (g4 == 0) lds_write_b32(sum_addr + wave * 64, psum);
      Fmt::p_write(pw_addr, pb);
    }
    lds_barrier();

    // ---- O^T += V^T P^T on this wave's 64 columns, all groups
    {
      float ws[NQ];
      lds_read_f32<NQ>(sum_addr, ws);
#pragma unroll
      for (int g = 0; g < G; ++g) {   // pairs of subtiles first: (ws0 + ws1) + (ws2 + ws3)
        float ts = ws[g] + ws[g + G];
#pragma unroll
        for (int s = 2; s < NSUB; s += 2) ts += ws[g + s * G] + ws[g + (s + 1) * G];
        l[g] += ts;
      }
    }
    Fmt::template pv<G>(pr_addr, v_addr + so, acc);
  };

  int stage = 0;
  for (int t = 0; t < ntiles; t += 2) {
    step(t, stage, pgA, pgB);
    stage = stage + 1 == MLA_NST ? 0 : stage + 1;
    if (t + 1 >= ntiles) break;
    step(t + 1, stage, pgB, pgA);
    stage = stage + 1 == MLA_NST ? 0 : stage + 1;
  }

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the two tiles staged past the end

  // ---- lane holds 16 columns of O^T[.][head c16] of every group, in units of the cache's scale
  const int64_t rows = (int64_t)B * H * S;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int head = h0 + g * 16 + c16;
    if (head >= H) continue;
    const float inv = kvs / l[g];
    const int64_t row = ((int64_t)b * H + head) * S + split;
    if (S > 1 && wave == 0 && g4 == 0) Fmt::scratch_of(fl)[rows * MLA_DV + row] = (m[g] + __log2f(l[g])) * kLn2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int col;
      const f32x4 v = Fmt::out4(acc[g], i, wave, g4, col) * inv;
      if (S > 1) {
        *reinterpret_cast<f32x4*>(Fmt::scratch_of(fl) + row * MLA_DV + col) = v;
      } else {
        T* op = o + b * o_sb + head * o_sh + col;
        Vec<T, 4> pk;
#pragma unroll
        for (int r = 0; r < 4; ++r) pk.v[r] = from_f32<T>(v[r]);
        if (o_vec) {
          *reinterpret_cast<Vec<T, 4>*>(op) = pk;
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) op[r] = pk.v[r];
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// merge of the splits (stage 2 of the reference): one workgroup per (sequence, head), 4 columns a thread
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(128) void mla_merge_kernel(T* __restrict__ o, const float* __restrict__ scratch,
                                                        const int* __restrict__ seq_lens, int B, int H, int S,
                                                        int64_t o_sb, int64_t o_sh, int o_vec) {
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int len = seq_lens[b];
  const int col = threadIdx.x * 4;
  const float* lse = scratch + (int64_t)B * H * S * MLA_DV + (int64_t)bh * S;
  const float* part = scratch + (int64_t)bh * S * MLA_DV + col;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float mx = -INFINITY, sum = 0.f;
  const int L = len > 0 ? (len + S - 1) / S : 1;
  for (int s = 0; s < S && s * L < len; ++s) {   // the non-empty splits
    const float e = lse[s];
    const f32x4 v = *reinterpret_cast<const f32x4*>(part + (int64_t)s * MLA_DV);
    const float nm = fmaxf(mx, e);
    const float sc = fast_exp2((mx - nm) * kLog2e), w = fast_exp2((e - nm) * kLog2e);
    acc = acc * sc + v * w;
    sum = sum * sc + w;
    mx = nm;
  }
  const float inv = len > 0 ? 1.0f / sum : 0.f;
  T* op = o + b * o_sb + h * o_sh + col;
  Vec<T, 4> pk;
#pragma unroll
  for (int r = 0; r < 4; ++r) pk.v[r] = from_f32<T>(acc[r] * inv);
  if (o_vec) {
    *reinterpret_cast<Vec<T, 4>*>(op) = pk;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) op[r] = pk.v[r];
  }
}

}  // namespace va

using namespace va;

template <typename T, typename Fmt>
static void launch_mla(void* o, const void* q, const void* cache, const int* bt, const int* sl, float* scratch,
                       const float* kv_scale, int B, int H, int S, int page_size, int max_blocks, float sm_scale,
                       int64_t q_sb, int64_t q_sh, int64_t o_sb, int64_t o_sh, int64_t c_sb, int64_t c_se,
                       int64_t bt_s, hipStream_t st) {
  // heads per workgroup: 32 once there are more than 16 (the widest variant that compiles without
  // spilling, see the header); "mla_hpw" forces a variant
  int hpw = H <= 16 ? 16 : 32;
  if (g_mla_hpw == 16 || g_mla_hpw == 32) hpw = g_mla_hpw;
  const int NC = ceil_div(H, hpw);
  const uint32_t ps_magic = page_size == 1 ? 0xffffffffu : (uint32_t)((1ull << 32) / (uint32_t)page_size);
  const int o_vec = (o_sb % 4 == 0 && o_sh % 4 == 0 && (((uintptr_t)o) & 7) == 0) ? 1 : 0;
  const unsigned grid = (unsigned)(ceil_div(B * S, 8) * NC * 8);
#define ML(G)                                                                                                    \
  hipLaunchKernelGGL((mla_decode_kernel<T, Fmt, G>), dim3(grid), dim3(MLA_NT), 0, st, (T*)o, (const T*)q,        \
                     (const typename Fmt::elem*)cache, bt, sl, Fmt::floats(scratch, kv_scale), B, H, S,           \
                     NC, page_size, ps_magic, max_blocks, sm_scale * kLog2e, q_sb, q_sh, o_sb, o_sh, c_sb, c_se,  \
                     bt_s, o_vec)
  if (hpw == 16) ML(1); else ML(2);
#undef ML
  if (S > 1)
    hipLaunchKernelGGL((mla_merge_kernel<T>), dim3(B * H), dim3(128), 0, st, (T*)o, (const float*)scratch, sl, B, H, S,
                       o_sb, o_sh, o_vec);
}

// The checks that do not depend on the cache format, in the order both entry points have always made
// them (a call with two faults keeps its message).  An entry point decides its own early rules and
// hands over the outcome, so that each is reported at its old place: other_call, null when kv_dtype is
// this call's, else the hint at the call that serves it; whether the cache's dtype is acceptable; and
// whether the pointers only this format has are set.  batch == 0 returns OK before any pointer is looked
// at: the caller then has nothing to launch.
static int mla_validate(const char* op, const char* form, const char* other_call, bool cache_dtype_ok,
                        bool own_ptrs, const void* o, const void* q, const void* kv_cache, const void* block_table,
                        const void* seq_lens, const float* attn_logits, int64_t attn_logits_floats, int batch,
                        int num_heads, int qk_width, int v_width, int page_size, int max_blocks_per_seq,
                        int num_kv_splits, int dtype, int cache_dtype, int index_bits) {
  VA_REQUIRE(batch >= 0 && num_heads >= 1 && page_size >= 1 && max_blocks_per_seq >= 1, VLLM_AMD_EINVAL,
             "%s: bad shape", op);
  VA_REQUIRE(qk_width == MLA_DK && v_width == MLA_DV, VLLM_AMD_EUNSUPPORTED,
             "%s: row width %d / %d is not supported; the supported form is %s", op, qk_width, v_width, form);
  VA_REQUIRE(!other_call, VLLM_AMD_EUNSUPPORTED, "%s: %s; the supported form is %s", op, other_call, form);
  VA_REQUIRE(dtype == VLLM_AMD_BF16 || dtype == VLLM_AMD_F16, VLLM_AMD_EUNSUPPORTED,
             "%s: q must be bfloat16 or float16; the supported form is %s", op, form);
  VA_REQUIRE(cache_dtype_ok, VLLM_AMD_EUNSUPPORTED,
             "%s: q and cache dtype mismatch (%d vs %d); the supported form is %s", op, dtype, cache_dtype, form);
  VA_REQUIRE(index_bits == 32, VLLM_AMD_EUNSUPPORTED, "%s: block table and seq_lens must be int32 (got %d-bit)", op,
             index_bits);
  VA_REQUIRE(num_kv_splits >= 1, VLLM_AMD_EINVAL, "%s: num_kv_splits %d < 1", op, num_kv_splits);
  VA_REQUIRE(num_heads <= 128, VLLM_AMD_EUNSUPPORTED, "%s: num_heads %d > 128", op, num_heads);
  const int64_t need = (int64_t)batch * num_heads * num_kv_splits * (MLA_DV + 1);
  VA_REQUIRE(num_kv_splits == 1 || attn_logits_floats >= need, VLLM_AMD_EINVAL,
             "%s: attn_logits scratch too small: %lld floats, [B, H, num_kv_splits, 513] needs %lld", op,
             (long long)attn_logits_floats, (long long)need);
  VA_REQUIRE((int64_t)batch * num_kv_splits < (1ll << 27), VLLM_AMD_EINVAL, "%s: batch * num_kv_splits too large", op);
  if (batch == 0) return VLLM_AMD_OK;
  VA_REQUIRE(o && q && kv_cache && block_table && seq_lens && own_ptrs && (num_kv_splits == 1 || attn_logits),
             VLLM_AMD_EINVAL, "%s: null pointer", op);
  return VLLM_AMD_OK;
}

#define MLA_LAUNCH(T, Fmt, kv_scale)                                                                              \
  launch_mla<T, Fmt<T>>(o, q, kv_cache, (const int*)block_table, (const int*)seq_lens, attn_logits, kv_scale, batch, \
                        num_heads, num_kv_splits, page_size, max_blocks_per_seq, sm_scale, q_stride_b, q_stride_h,  \
                        o_stride_b, o_stride_h, cache_block_stride, cache_entry_stride, block_table_stride,         \
                        (hipStream_t)stream)

extern "C" int vllm_amd_mla_decode(void* o, const void* q, const void* kv_cache, const void* block_table,
                                   const void* seq_lens, float* attn_logits, int64_t attn_logits_floats, int batch,
                                   int num_heads, int qk_width, int v_width, int page_size,
                                   int max_blocks_per_seq, int num_kv_splits, float sm_scale, int64_t q_stride_b,
                                   int64_t q_stride_h, int64_t o_stride_b, int64_t o_stride_h,
                                   int64_t cache_block_stride, int64_t cache_entry_stride,
                                   int64_t block_table_stride, int dtype, int cache_dtype, int kv_dtype,
                                   int index_bits, void* stream) {
  const char* op = "mla_decode";
  const char* form = "q [B, H, 576] and a [num_blocks, page_size, 576] latent cache of the same bfloat16 / float16 "
                     "type (kv_cache_dtype \"auto\"), v = its first 512 columns, int32 block table and lengths";
  const char* other_call = kv_dtype == VLLM_AMD_KV_AUTO ? nullptr
      : "an fp8 latent cache goes through the scaled call, vllm_amd_mla_decode_fp8 (decode_attention_fwd with "
        "k_scale), not this one";
  const int rc = mla_validate(op, form, other_call, cache_dtype == dtype, true, o, q, kv_cache, block_table, seq_lens,
                              attn_logits, attn_logits_floats, batch, num_heads, qk_width, v_width, page_size,
                              max_blocks_per_seq, num_kv_splits, dtype, cache_dtype, index_bits);
  if (rc != VLLM_AMD_OK || batch == 0) return rc;
  VA_REQUIRE(q_stride_b % 8 == 0 && q_stride_h % 8 == 0 && cache_block_stride % 8 == 0 &&
                 cache_entry_stride % 8 == 0 && cache_entry_stride >= MLA_DK && (((uintptr_t)q) & 15) == 0 &&
                 (((uintptr_t)kv_cache) & 15) == 0 && (((uintptr_t)attn_logits) & 15) == 0,
             VLLM_AMD_EUNSUPPORTED, "%s: q / cache strides must be multiples of 8 elements and q, cache, attn_logits "
             "16-byte aligned", op);
  if (dtype == VLLM_AMD_BF16) MLA_LAUNCH(bf16_t, MlaRows16, nullptr); else MLA_LAUNCH(f16_t, MlaRows16, nullptr);
  VA_LAUNCH_CHECK("mla_decode launch");
  return VLLM_AMD_OK;
}

// the fp8 cache: the same grid and heads-per-workgroup rule, the same merge; cache_dtype is not looked at
extern "C" int vllm_amd_mla_decode_fp8(void* o, const void* q, const void* kv_cache, const void* block_table,
                                       const void* seq_lens, float* attn_logits, int64_t attn_logits_floats,
                                       int batch, int num_heads, int qk_width, int v_width, int page_size,
                                       int max_blocks_per_seq, int num_kv_splits, float sm_scale,
                                       int64_t q_stride_b, int64_t q_stride_h, int64_t o_stride_b,
                                       int64_t o_stride_h, int64_t cache_block_stride, int64_t cache_entry_stride,
                                       int64_t block_table_stride, int dtype, int cache_dtype, int kv_dtype,
                                       int index_bits, const float* kv_scale, void* stream) {
  const char* op = "mla_decode_fp8";
  const char* form = "bfloat16 / float16 q [B, H, 576] and a [num_blocks, page_size, 576] latent cache of e4m3fn "
                     "bytes (kv_cache_dtype \"fp8\" / \"fp8_e4m3\") with its scale as a device float[1], v = its "
                     "first 512 columns, byte strides that are multiples of 16, int32 block table and lengths";
  const char* other_call =
      kv_dtype == VLLM_AMD_KV_FP8_E4M3 ? nullptr : "a 16-bit latent cache goes through vllm_amd_mla_decode";
  const int rc = mla_validate(op, form, other_call, true, kv_scale != nullptr, o, q, kv_cache, block_table, seq_lens,
                              attn_logits, attn_logits_floats, batch, num_heads, qk_width, v_width, page_size,
                              max_blocks_per_seq, num_kv_splits, dtype, cache_dtype, index_bits);
  if (rc != VLLM_AMD_OK || batch == 0) return rc;
  VA_REQUIRE(q_stride_b % 8 == 0 && q_stride_h % 8 == 0 && (((uintptr_t)q) & 15) == 0 &&
                 (((uintptr_t)attn_logits) & 15) == 0,
             VLLM_AMD_EUNSUPPORTED, "%s: q strides must be multiples of 8 elements and q, attn_logits 16-byte aligned",
             op);
  VA_REQUIRE(cache_block_stride % 16 == 0 && cache_entry_stride % 16 == 0 && cache_entry_stride >= MLA_DK &&
                 (((uintptr_t)kv_cache) & 15) == 0,
             VLLM_AMD_EUNSUPPORTED, "%s: cache strides (%lld / %lld bytes) must be multiples of 16, the entry stride "
             ">= 576 and the cache 16-byte aligned; the supported form is %s", op, (long long)cache_block_stride,
             (long long)cache_entry_stride, form);
  if (dtype == VLLM_AMD_BF16) MLA_LAUNCH(bf16_t, MlaRowsFp8, kv_scale); else MLA_LAUNCH(f16_t, MlaRowsFp8, kv_scale);
  VA_LAUNCH_CHECK("mla_decode_fp8 launch");
  return VLLM_AMD_OK;
}
