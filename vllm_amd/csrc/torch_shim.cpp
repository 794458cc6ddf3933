// PyTorch-ROCm operator shim over the C ABI (include/vllm_amd.h): the C++ side of
// torch.ops._C / _C_cache_ops / _rocm_C / _moe_C for the hot path, registered with the reference's
// schema strings (csrc/torch_bindings.cpp:45-69, 117-120, 188-211, 422-427, 575-593, 676-708;
// csrc/rocm/torch_bindings.cpp:34-56; csrc/moe/torch_bindings.cpp:13-22).  Every implementation
// unpacks data_ptr / sizes / strides, takes torch's current HIP stream and calls libvllm_amd.so; a non-zero status
// becomes the c10::Error (RuntimeError) the reference's TORCH_CHECK raises.  No tensor is
// allocated inside an op, except the one-time per-device workspace (ensure_workspace).
//
// Registration is a function (vllm_amd_torch_register), not a static TORCH_LIBRARY block:
// when the real vLLM extension was imported first its schemas already exist, and a static
// m.def() would abort the process at dlopen; here a duplicate definition is skipped and only
// the kernel for the CUDA(=HIP) key is (re)registered.
#include <torch/library.h>
#include <ATen/core/Tensor.h>
#include <ATen/ops/empty.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <vector>

#include "../../include/vllm_amd.h"

namespace {

using at::Tensor;
using OptTensor = std::optional<Tensor>;
using DevGuard = at::hip::OptionalHIPGuardMasqueradingAsCUDA;

inline void check(int rc) { TORCH_CHECK(rc == 0, vllm_amd_last_error()); }

inline void* stream_of(const Tensor& t) {
  return (void*)c10::hip::getCurrentHIPStream(t.get_device()).stream();
}

inline void need_dev(const Tensor& t) {
  TORCH_CHECK(t.is_cuda(), "vllm_amd ops need device tensors (cuda/HIP); got ", t.device());
}
inline void need_dev(const OptTensor& t) { if (t.has_value()) need_dev(*t); }
template <class... Ts> inline void need_devs(const Ts&... ts) { (need_dev(ts), ...); }

inline int dt(const Tensor& t) {
  switch (t.scalar_type()) {
    case at::kFloat: return VLLM_AMD_F32;
    case at::kHalf: return VLLM_AMD_F16;
    case at::kBFloat16: return VLLM_AMD_BF16;
    default: TORCH_CHECK(false, "Unsupported data type: ", t.scalar_type());
  }
}
inline bool is_fp8(const Tensor& t) {
  return t.scalar_type() == at::kByte || t.scalar_type() == at::kFloat8_e4m3fn;
}
inline bool is_16_32(const Tensor& t) {
  return t.scalar_type() == at::kFloat || t.scalar_type() == at::kHalf || t.scalar_type() == at::kBFloat16;
}
// csrc/quantization/fp8/amd/quant_utils.cuh:641-667
inline int kv(const std::string& s) {
  if (s == "auto") return VLLM_AMD_KV_AUTO;
  if (s == "fp8" || s == "fp8_e4m3") return VLLM_AMD_KV_FP8_E4M3;
  TORCH_CHECK(false, "Unsupported data type of kv cache: ", s);
}
inline const float* fptr(const Tensor& t) { return (const float*)t.data_ptr(); }
inline const float* fptr(const OptTensor& t) { return t.has_value() ? (const float*)t->data_ptr() : nullptr; }
inline void* vptr(const OptTensor& t) { return t.has_value() ? t->data_ptr() : nullptr; }

// ---- the library workspace (vllm_amd_set_workspace) --------------------------------------
// The C ABI allocates nothing, so this layer owns one buffer per device (4 stream slots x 16 MiB
// + ticket counters) and registers it once, outside stream capture, before that device's first
// scaled_mm -- and before its first paged_attention_v1 only when the balanced form ("pa_balance" = 1,
// off by default) is on: nothing else of that op uses it.  Without it the GEMM never splits over K.
// One host synchronisation, in that first call.  Launches under stream capture never take a workspace
// slot, so a captured GEMM runs unsplit: split-K (M <= 64, K >= 12288: 17.2 -> 15.2 us) is an
// eager-launch optimisation; bench.py's graph-timed GEMM legs time the unsplit form.
constexpr int64_t kWsBytes = (64ll << 20) + (512ll << 10);
std::mutex g_ws_mu;
Tensor g_ws[64];
std::atomic<bool> g_ws_set[64];

void ensure_workspace(const Tensor& t) {
  const int idx = t.get_device();
  if (idx < 0 || idx >= 64 || g_ws_set[idx].load(std::memory_order_acquire)) return;
  std::lock_guard<std::mutex> lk(g_ws_mu);
  if (g_ws_set[idx].load(std::memory_order_relaxed)) return;
  hipStream_t s = c10::hip::getCurrentHIPStream(idx).stream();
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &st) != hipSuccess || st != hipStreamCaptureStatusNone) {
    (void)hipGetLastError();
    return;   // not during capture; the next eager call registers it
  }
  DevGuard g(t.device());
  g_ws[idx] = at::empty({kWsBytes}, t.options().dtype(at::kByte));
  check(vllm_amd_set_workspace(g_ws[idx].data_ptr(), kWsBytes, (void*)s));
  // every stream's first launch must see the zeroed counters
  TORCH_CHECK(hipStreamSynchronize(s) == hipSuccess, "hipStreamSynchronize failed");
  g_ws_set[idx].store(true, std::memory_order_release);
}

// ---- attention ---------------------------------------------------------------------------
void paged_attention_v1(Tensor& out, const Tensor& query, const Tensor& key_cache, const Tensor& value_cache,
                        int64_t num_kv_heads, double scale, const Tensor& block_tables, const Tensor& seq_lens,
                        int64_t block_size, int64_t max_seq_len, const OptTensor& alibi_slopes,
                        const std::string& kv_cache_dtype, const Tensor& k_scale, const Tensor& v_scale,
                        int64_t tp_rank, int64_t bs_local_blocks, int64_t bs_vert_stride, int64_t bs_block_size,
                        int64_t bs_head_sliding_step) {
  need_devs(out, query, key_cache, value_cache, block_tables, seq_lens, alibi_slopes, k_scale, v_scale);
  TORCH_CHECK(query.dim() == 3 && out.is_contiguous(), "out.is_contiguous() && query.dim() == 3");
  TORCH_CHECK(block_tables.scalar_type() == at::kInt && seq_lens.scalar_type() == at::kInt,
              "block_tables / seq_lens must be int32");
  {
    int bal = 0;   // only the balanced form (opt-in) uses the workspace
    if (vllm_amd_get_tuning("pa_balance", &bal) == VLLM_AMD_OK && bal == 1) ensure_workspace(query);
  }
  DevGuard g(query.device());
  check(vllm_amd_paged_attention_v1(
      out.data_ptr(), query.data_ptr(), key_cache.data_ptr(), value_cache.data_ptr(), (int)query.size(0),
      (int)query.size(1), (int)query.size(2), (int)num_kv_heads, (float)scale, (const int*)block_tables.data_ptr(),
      (const int*)seq_lens.data_ptr(), (int)block_tables.size(1), (int)block_size, (int)max_seq_len,
      fptr(alibi_slopes), dt(query), kv(kv_cache_dtype), fptr(k_scale), fptr(v_scale), query.stride(0),
      key_cache.stride(0), key_cache.stride(1), (int)tp_rank, (int)bs_local_blocks, (int)bs_vert_stride,
      (int)bs_block_size, (int)bs_head_sliding_step, stream_of(query)));
}

void paged_attention_v2(Tensor& out, Tensor& exp_sums, Tensor& max_logits, Tensor& tmp_out, const Tensor& query,
                        const Tensor& key_cache, const Tensor& value_cache, int64_t num_kv_heads, double scale,
                        const Tensor& block_tables, const Tensor& seq_lens, int64_t block_size, int64_t max_seq_len,
                        const OptTensor& alibi_slopes, const std::string& kv_cache_dtype, const Tensor& k_scale,
                        const Tensor& v_scale, int64_t tp_rank, int64_t bs_local_blocks, int64_t bs_vert_stride,
                        int64_t bs_block_size, int64_t bs_head_sliding_step) {
  need_devs(out, exp_sums, max_logits, tmp_out, query, key_cache, value_cache, block_tables, seq_lens,
            alibi_slopes, k_scale, v_scale);
  TORCH_CHECK(query.dim() == 3 && out.is_contiguous() && tmp_out.is_contiguous() && exp_sums.is_contiguous() &&
                  max_logits.is_contiguous(), "out / tmp_out / exp_sums / max_logits must be contiguous");
  TORCH_CHECK(exp_sums.scalar_type() == at::kFloat && max_logits.scalar_type() == at::kFloat,
              "exp_sums / max_logits must be float32");
  TORCH_CHECK(block_tables.scalar_type() == at::kInt && seq_lens.scalar_type() == at::kInt,
              "block_tables / seq_lens must be int32");
  DevGuard g(query.device());
  check(vllm_amd_paged_attention_v2(
      out.data_ptr(), (float*)exp_sums.data_ptr(), (float*)max_logits.data_ptr(), tmp_out.data_ptr(),
      query.data_ptr(), key_cache.data_ptr(), value_cache.data_ptr(), (int)query.size(0), (int)query.size(1),
      (int)query.size(2), (int)num_kv_heads, (float)scale, (const int*)block_tables.data_ptr(),
      (const int*)seq_lens.data_ptr(), (int)block_tables.size(1), (int)block_size, (int)max_seq_len,
      (int)exp_sums.size(-1), fptr(alibi_slopes), dt(query), kv(kv_cache_dtype), fptr(k_scale), fptr(v_scale),
      query.stride(0), key_cache.stride(0), key_cache.stride(1), (int)tp_rank, (int)bs_local_blocks,
      (int)bs_vert_stride, (int)bs_block_size, (int)bs_head_sliding_step, stream_of(query)));
}

void paged_attention_rocm(Tensor& out, const Tensor& exp_sums, const Tensor& max_logits, const Tensor& tmp_out,
                          const Tensor& query, const Tensor& key_cache, const Tensor& value_cache,
                          int64_t num_kv_heads, double scale, const Tensor& block_tables,
                          const Tensor& context_lens, const OptTensor& query_start_loc, int64_t block_size,
                          int64_t max_context_len, const OptTensor& alibi_slopes, const std::string& kv_cache_dtype,
                          const Tensor& k_scale, const Tensor& v_scale, const OptTensor& fp8_out_scale) {
  need_devs(out, exp_sums, max_logits, tmp_out, query, key_cache, value_cache, block_tables, context_lens,
            query_start_loc, alibi_slopes, k_scale, v_scale, fp8_out_scale);
  TORCH_CHECK(query.dim() == 3 && out.is_contiguous() && tmp_out.is_contiguous() && exp_sums.is_contiguous(),
              "out / tmp_out / exp_sums must be contiguous");
  TORCH_CHECK(block_tables.scalar_type() == at::kInt && context_lens.scalar_type() == at::kInt,
              "block_tables / context_lens must be int32");
  TORCH_CHECK(!query_start_loc.has_value() || query_start_loc->scalar_type() == at::kInt,
              "query_start_loc must be int32");
  DevGuard g(query.device());
  check(vllm_amd_paged_attention_rocm(
      out.data_ptr(), (float*)exp_sums.data_ptr(), (float*)max_logits.data_ptr(), tmp_out.data_ptr(),
      query.data_ptr(), key_cache.data_ptr(), value_cache.data_ptr(), (int)block_tables.size(0), (int)query.size(1),
      (int)query.size(2), (int)num_kv_heads, (float)scale, (const int*)block_tables.data_ptr(),
      (const int*)context_lens.data_ptr(), (const int*)vptr(query_start_loc), (int)block_tables.size(1),
      (int)block_size, (int)max_context_len, (int)exp_sums.size(-1), fptr(alibi_slopes), dt(query),
      kv(kv_cache_dtype), fptr(k_scale), fptr(v_scale), fptr(fp8_out_scale), query.stride(0), key_cache.stride(0),
      key_cache.stride(1), stream_of(query)));
}

// ---- cache ops ---------------------------------------------------------------------------
void reshape_and_cache(const Tensor& key, const Tensor& value, Tensor& key_cache, Tensor& value_cache,
                       const Tensor& slot_mapping, const std::string& kv_cache_dtype, const Tensor& k_scale,
                       const Tensor& v_scale) {
  need_devs(key, value, key_cache, value_cache, slot_mapping, k_scale, v_scale);
  const int64_t head_size = key.size(2);
  TORCH_CHECK(slot_mapping.scalar_type() == at::kLong && key.stride(2) == 1 && key.stride(1) == head_size,
              "slot_mapping must be int64 and key [num_tokens, num_heads, head_size] dense per token");
  DevGuard g(key.device());
  check(vllm_amd_reshape_and_cache(
      key.data_ptr(), value.data_ptr(), key_cache.data_ptr(), value_cache.data_ptr(),
      (const int64_t*)slot_mapping.data_ptr(), (int)slot_mapping.size(0), (int)key.size(1), (int)head_size,
      (int)key_cache.size(3), (int)key_cache.size(4), key.stride(0), value.stride(0), dt(key), kv(kv_cache_dtype),
      fptr(k_scale), fptr(v_scale), stream_of(key)));
}

void reshape_and_cache_flash(const Tensor& key, const Tensor& value, Tensor& key_cache, Tensor& value_cache,
                             const Tensor& slot_mapping, const std::string& kv_cache_dtype, const Tensor& k_scale,
                             const Tensor& v_scale) {
  need_devs(key, value, key_cache, value_cache, slot_mapping, k_scale, v_scale);
  const int64_t head_size = key.size(2);
  TORCH_CHECK(slot_mapping.scalar_type() == at::kLong && key.stride(2) == 1 && key.stride(1) == head_size,
              "slot_mapping must be int64 and key [num_tokens, num_heads, head_size] dense per token");
  TORCH_CHECK(key_cache.stride(0) == value_cache.stride(0), "key_cache.stride(0) == value_cache.stride(0)");  // cache_kernels.cu:441
  DevGuard g(key.device());
  check(vllm_amd_reshape_and_cache_flash(
      key.data_ptr(), value.data_ptr(), key_cache.data_ptr(), value_cache.data_ptr(),
      (const int64_t*)slot_mapping.data_ptr(), (int)slot_mapping.size(0), (int)key.size(1), (int)head_size,
      (int)key_cache.size(1), key.stride(0), value.stride(0), key_cache.stride(0), key_cache.stride(1),
      key_cache.stride(2), dt(key), kv(kv_cache_dtype), fptr(k_scale), fptr(v_scale), stream_of(key)));
}

// csrc/cache_kernels.cu:465-501
void concat_and_cache_mla(const Tensor& kv_c, const Tensor& k_pe, Tensor& kv_cache, const Tensor& slot_mapping,
                          const std::string& kv_cache_dtype, const Tensor& scale) {
  need_devs(kv_c, k_pe, kv_cache, slot_mapping, scale);
  TORCH_CHECK(kv_c.dim() == 2 && k_pe.dim() == 2 && kv_cache.dim() == 3 && kv_c.stride(1) == 1 && k_pe.stride(1) == 1 &&
                  kv_cache.stride(2) == 1 && slot_mapping.scalar_type() == at::kLong && slot_mapping.is_contiguous(),
              "concat_and_cache_mla: kv_c [T, rank], k_pe [T, pe], kv_cache [blocks, block_size, rank + pe] with "
              "contiguous rows and an int64 slot_mapping are required");
  TORCH_CHECK(kv_cache.size(2) == kv_c.size(1) + k_pe.size(1), "kv_cache.size(2) == kv_lora_rank + pe_dim");  // :487
  TORCH_CHECK(slot_mapping.size(0) <= kv_c.size(0) && slot_mapping.size(0) <= k_pe.size(0),
              "concat_and_cache_mla: slot_mapping is longer than kv_c / k_pe");
  TORCH_CHECK(k_pe.scalar_type() == kv_c.scalar_type(), "concat_and_cache_mla: kv_c and k_pe differ in dtype");
  const int kvd = kv(kv_cache_dtype);
  if (kvd == VLLM_AMD_KV_AUTO) {
    TORCH_CHECK(kv_cache.scalar_type() == kv_c.scalar_type(), "concat_and_cache_mla: \"auto\" needs a cache of kv_c's dtype");
  } else {
    TORCH_CHECK(is_fp8(kv_cache) && scale.scalar_type() == at::kFloat,
                "concat_and_cache_mla: fp8 needs a byte cache and a float scale");
  }
  DevGuard g(kv_c.device());
  check(vllm_amd_concat_and_cache_mla(kv_c.data_ptr(), k_pe.data_ptr(), kv_cache.data_ptr(),
                                      (const int64_t*)slot_mapping.data_ptr(), (int)slot_mapping.size(0),
                                      (int)kv_c.size(1), (int)k_pe.size(1), (int)kv_cache.size(1), kv_c.stride(0),
                                      k_pe.stride(0), kv_cache.stride(0), kv_cache.stride(1), dt(kv_c), kvd,
                                      fptr(scale), stream_of(kv_c)));
}

void convert_fp8(Tensor& dst_cache, const Tensor& src_cache, double scale, const std::string& kv_cache_dtype) {
  need_devs(dst_cache, src_cache);
  (void)kv(kv_cache_dtype);   // validates the string; "auto" is treated as e4m3 (gfx950 has one fp8 KV type)
  int to_fp8, d;
  if (is_16_32(src_cache) && is_fp8(dst_cache)) { to_fp8 = 1; d = dt(src_cache); }
  else if (is_fp8(src_cache) && is_16_32(dst_cache)) { to_fp8 = 0; d = dt(dst_cache); }
  else TORCH_CHECK(false, "Unsupported data type: ", src_cache.scalar_type(), " -> ", dst_cache.scalar_type());
  TORCH_CHECK(src_cache.is_contiguous() && dst_cache.is_contiguous(), "convert_fp8: contiguous tensors required");
  DevGuard g(src_cache.device());
  check(vllm_amd_convert_fp8(dst_cache.data_ptr(), src_cache.data_ptr(), src_cache.numel(), (float)scale, d, to_fp8,
                             stream_of(src_cache)));
}

// csrc/cache_kernels.cu:675-734 (same-dtype copy; the fp8-widening form is reached through the C ABI only)
void gather_cache(const Tensor& src_cache, Tensor& dst, const Tensor& block_table, const Tensor& cu_seq_lens,
                  int64_t batch_size, const OptTensor& seq_starts) {
  need_devs(src_cache, dst, block_table, cu_seq_lens, seq_starts);
  TORCH_CHECK(block_table.scalar_type() == at::kInt, "block_table must be int32");
  TORCH_CHECK(cu_seq_lens.scalar_type() == at::kInt, "cu_seq_lens must be int32");
  TORCH_CHECK(!seq_starts.has_value() || seq_starts->scalar_type() == at::kInt, "seq_starts must be int32");
  TORCH_CHECK(src_cache.scalar_type() == dst.scalar_type(), "src_cache and dst must have the same dtype");
  TORCH_CHECK(src_cache.dim() >= 3 && dst.dim() >= 2, "gather_cache: src_cache [NUM_BLOCKS, BLOCK_SIZE, ENTRIES...], dst [TOT_TOKENS, ENTRIES...]");
  const int64_t entry = src_cache.numel() == 0 ? 0 : src_cache.numel() / (src_cache.size(0) * src_cache.size(1));
  TORCH_CHECK(entry > 0 && dst.numel() == dst.size(0) * entry && src_cache[0][0].is_contiguous() &&
                  (dst.size(0) == 0 || dst[0].is_contiguous()) && block_table.dim() == 2 && block_table.stride(1) == 1 &&
                  cu_seq_lens.is_contiguous() && cu_seq_lens.numel() > batch_size &&
                  (!seq_starts.has_value() || (seq_starts->is_contiguous() && seq_starts->numel() >= batch_size)),
              "gather_cache: entries of src_cache and dst must be contiguous and of one size; block_table [BATCH, "
              "BLOCK_INDICES], cu_seq_lens [BATCH + 1], seq_starts [BATCH]");
  DevGuard g(src_cache.device());
  check(vllm_amd_gather_cache(src_cache.data_ptr(), dst.data_ptr(), (const int32_t*)block_table.data_ptr(),
                              (const int32_t*)cu_seq_lens.data_ptr(), (const int32_t*)vptr(seq_starts), (int)batch_size,
                              dst.size(0), (int)src_cache.size(1), (int)entry, block_table.stride(0),
                              src_cache.stride(0), src_cache.stride(1), dst.stride(0), (int)src_cache.element_size(),
                              VLLM_AMD_F32, VLLM_AMD_KV_AUTO, nullptr, stream_of(src_cache)));
}

// csrc/cache_kernels.cu:123-170; one launch per layer (no pointer table upload, no sync)
void copy_blocks(const std::vector<Tensor>& key_caches, const std::vector<Tensor>& value_caches,
                 const Tensor& block_mapping) {
  TORCH_CHECK(key_caches.size() == value_caches.size(), "num_layers == value_caches.size()");
  if (key_caches.empty()) return;
  need_dev(block_mapping);
  TORCH_CHECK(block_mapping.scalar_type() == at::kLong && block_mapping.is_contiguous(),
              "block_mapping must be a contiguous int64 tensor");
  const int num_pairs = (int)block_mapping.size(0);
  for (size_t i = 0; i < key_caches.size(); i++) {
    const Tensor& kc = key_caches[i];
    const Tensor& vc = value_caches[i];
    need_devs(kc, vc);
    DevGuard g(kc.device());
    check(vllm_amd_copy_blocks(kc.data_ptr(), vc.data_ptr(), (const int64_t*)block_mapping.data_ptr(), num_pairs,
                               kc.stride(0) * (int64_t)kc.element_size(), stream_of(kc)));
  }
}

// csrc/cache_kernels.cu:25-67: per-pair async copies on the current stream of the device side;
// block_mapping lives on the CPU
void swap_blocks(const Tensor& src, Tensor& dst, const Tensor& block_mapping) {
  TORCH_CHECK(block_mapping.device().is_cpu(), "block_mapping must be on CPU");
  TORCH_CHECK(!(src.is_cuda() && dst.is_cuda()) || src.device() == dst.device(),
              "src and dst must be on the same GPU");
  TORCH_CHECK(src.is_cuda() || dst.is_cuda(), "Invalid device combination");
  Tensor bm = block_mapping.to(at::kLong).contiguous();
  const Tensor& gpu = src.is_cuda() ? src : dst;
  DevGuard g(gpu.device());
  check(vllm_amd_swap_blocks(src.data_ptr(), dst.data_ptr(), (int64_t)src.element_size() * src.stride(0),
                             (const int64_t*)bm.data_ptr(), bm.size(0), stream_of(gpu)));
}

// ---- fp8 quantisation --------------------------------------------------------------------
inline void fp8_out(const Tensor& result) {
  TORCH_CHECK(is_fp8(result), "Unsupported fp8 type: ", result.scalar_type());
  TORCH_CHECK(result.is_contiguous(), "out.is_contiguous()");
}
inline int64_t rows_of(const Tensor& input, int64_t hidden) { return hidden ? input.numel() / hidden : 0; }

inline int64_t quant_common(const Tensor& result, const Tensor& input) {
  need_devs(result, input);
  TORCH_CHECK(input.is_contiguous(), "input.is_contiguous()");
  TORCH_CHECK(result.is_contiguous(), "out.is_contiguous()");
  TORCH_CHECK(is_fp8(result), "Unsupported fp8 type: ", result.scalar_type());
  return rows_of(input, input.size(-1));
}

void static_scaled_fp8_quant(Tensor& result, const Tensor& input, const Tensor& scale) {
  const int64_t nt = quant_common(result, input);
  DevGuard g(input.device());
  check(vllm_amd_static_scaled_fp8_quant(result.data_ptr(), input.data_ptr(), fptr(scale), nt, (int)input.size(-1),
                                         dt(input), stream_of(input)));
}

void dynamic_scaled_fp8_quant(Tensor& result, const Tensor& input, Tensor& scale) {
  const int64_t nt = quant_common(result, input);
  DevGuard g(input.device());
  check(vllm_amd_dynamic_scaled_fp8_quant(result.data_ptr(), input.data_ptr(), (float*)scale.data_ptr(), nt,
                                          (int)input.size(-1), dt(input), stream_of(input)));
}

void dynamic_per_token_scaled_fp8_quant(Tensor& result, const Tensor& input, Tensor& scale,
                                        const OptTensor& scale_ub) {
  const int64_t nt = quant_common(result, input);
  DevGuard g(input.device());
  check(vllm_amd_dynamic_per_token_scaled_fp8_quant(result.data_ptr(), input.data_ptr(), (float*)scale.data_ptr(),
                                                    fptr(scale_ub), nt, (int)input.size(-1), dt(input),
                                                    stream_of(input)));
}

// csrc/quantization/fp8/per_token_group_quant.cu:121-217
void per_token_group_fp8_quant(const Tensor& input, Tensor& output_q, Tensor& output_s, int64_t group_size, double eps,
                               double fp8_min, double fp8_max, bool scale_ue8m0) {
  need_devs(input, output_q, output_s);
  TORCH_CHECK(input.is_contiguous(), "input.is_contiguous()");
  TORCH_CHECK(output_q.is_contiguous(), "output_q.is_contiguous()");
  TORCH_CHECK(is_fp8(output_q), "Unsupported fp8 type: ", output_q.scalar_type());
  TORCH_CHECK(group_size > 0 && input.dim() >= 1 && input.size(-1) % group_size == 0 &&
                  output_q.numel() == input.numel(),
              "input.numel() % group_size == 0");
  const int64_t hidden = input.size(-1), nt = rows_of(input, hidden), groups = hidden / group_size;
  TORCH_CHECK(output_s.dim() == 2 && output_s.scalar_type() == at::kFloat && output_s.size(0) == nt &&
                  output_s.size(1) == groups,
              "output_s.dim() == 2 (float32 [num_tokens, hidden / group_size])");
  DevGuard g(input.device());
  check(vllm_amd_per_token_group_fp8_quant(output_q.data_ptr(), (float*)output_s.data_ptr(), input.data_ptr(), nt,
                                           (int)hidden, (int)group_size, (float)eps, (float)fp8_min, (float)fp8_max,
                                           scale_ue8m0 ? 1 : 0, output_s.stride(0), output_s.stride(1), dt(input),
                                           stream_of(input)));
}

// ---- GEMM --------------------------------------------------------------------------------
// csrc/quantization/cutlass_w8a8/scaled_mm_entry.cu checks, restated
void cutlass_scaled_mm(Tensor& out, const Tensor& a, const Tensor& b, const Tensor& a_scales,
                       const Tensor& b_scales, const OptTensor& bias) {
  need_devs(out, a, b, a_scales, b_scales, bias);
  ensure_workspace(a);
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && out.dim() == 2, "a.dim() == 2 && b.dim() == 2 && c.dim() == 2");
  const int64_t M = a.size(0), K = a.size(1), N = b.size(1);
  TORCH_CHECK(out.size(0) == M && b.size(0) == K && out.size(1) == N,
              "c.size(0) == a.size(0) && a.size(1) == b.size(0) && b.size(1) == c.size(1)");
  TORCH_CHECK(a.stride(1) == 1 && out.stride(1) == 1, "a.stride(1) == 1 && c.stride(1) == 1");  // row major
  TORCH_CHECK(b.stride(0) == 1, "b.stride(0) == 1");                                             // column major
  TORCH_CHECK(is_fp8(a) && is_fp8(b), "scaled_mm: only fp8 e4m3 x fp8 e4m3 is implemented on gfx950");
  TORCH_CHECK(a_scales.scalar_type() == at::kFloat && b_scales.scalar_type() == at::kFloat,
              "scales must be float32");
  TORCH_CHECK(!bias.has_value() || (bias->numel() == N && bias->is_contiguous() && bias->dim() == 1 &&
                                    bias->scalar_type() == out.scalar_type()),
              "bias.numel() == b.size(1) && bias.is_contiguous() && bias.dim() == 1");
  DevGuard g(a.device());
  // per-tensor / per-token / per-channel scales first; the only shapes that are also group scales have
  // K = 128, where both rules mean the same product
  const bool plain = (a_scales.numel() == 1 || a_scales.numel() == M) && (b_scales.numel() == 1 || b_scales.numel() == N);
  if (!plain) {
    // group broadcast (vllm/_custom_ops.py:709-723): a_scales [M, K/128], b_scales [K/128, ceil(N/128)], any strides
    const int64_t kb = K / 128, nb = (N + 127) / 128;
    TORCH_CHECK(K % 128 == 0 && a_scales.dim() == 2 && b_scales.dim() == 2 && a_scales.size(0) == M &&
                    a_scales.size(1) == kb && b_scales.size(0) == kb && b_scales.size(1) == nb,
                "cutlass_scaled_mm: scales must be per-tensor ([1]), per-token / per-channel (a_scales [M, 1], "
                "b_scales [N, 1]), or blockwise (a_scales [M, K/128], b_scales [K/128, ceil(N/128)]); got a_scales ",
                a_scales.sizes(), ", b_scales ", b_scales.sizes(), " for M, N, K = ", M, ", ", N, ", ", K);
    check(vllm_amd_scaled_mm_blockwise(out.data_ptr(), a.data_ptr(), b.data_ptr(), fptr(a_scales), fptr(b_scales),
                                       vptr(bias), (int)M, (int)N, (int)K, a.stride(0), b.stride(1), out.stride(0),
                                       a_scales.stride(0), a_scales.stride(1), b_scales.stride(0), b_scales.stride(1),
                                       dt(out), stream_of(a)));
    return;
  }
  TORCH_CHECK(a_scales.is_contiguous() && b_scales.is_contiguous(),
              "a_scales.is_contiguous() && b_scales.is_contiguous()");
  check(vllm_amd_scaled_mm(out.data_ptr(), a.data_ptr(), b.data_ptr(), fptr(a_scales), fptr(b_scales), vptr(bias),
                           (int)M, (int)N, (int)K, a.stride(0), b.stride(1), out.stride(0), (int)a_scales.numel(),
                           (int)b_scales.numel(), dt(out), stream_of(a)));
}

// ---- fused MoE over block-scaled fp8 weights (csrc/moe_block_fp8.hip) ------------------------
inline bool is_i32(const Tensor& t) { return t.scalar_type() == at::kInt && t.is_contiguous(); }

// csrc/moe/moe_align_sum_kernels.cu (moe_align_block_size)
void moe_align_block_size(const Tensor& topk_ids, int64_t num_experts, int64_t block_size, Tensor& sorted_token_ids,
                          Tensor& experts_ids, Tensor& num_tokens_post_pad) {
  need_devs(topk_ids, sorted_token_ids, experts_ids, num_tokens_post_pad);
  TORCH_CHECK(is_i32(topk_ids) && is_i32(sorted_token_ids) && is_i32(experts_ids) && is_i32(num_tokens_post_pad),
              "moe_align_block_size: contiguous int32 tensors required");
  TORCH_CHECK(block_size > 0 && num_experts >= 0, "moe_align_block_size: block_size > 0 && num_experts >= 0");
  const int64_t max_padded = topk_ids.numel() + num_experts * (block_size - 1);
  TORCH_CHECK(sorted_token_ids.numel() >= max_padded &&
                  experts_ids.numel() >= (max_padded + block_size - 1) / block_size && num_tokens_post_pad.numel() >= 1,
              "moe_align_block_size: sorted_token_ids needs numel + num_experts * (block_size - 1) entries and "
              "experts_ids one per block of them");
  DevGuard g(topk_ids.device());
  check(vllm_amd_moe_align_block_size((const int32_t*)topk_ids.data_ptr(), topk_ids.numel(), (int)num_experts,
                                      (int)block_size, (int32_t*)sorted_token_ids.data_ptr(),
                                      (int32_t*)experts_ids.data_ptr(), (int32_t*)num_tokens_post_pad.data_ptr(),
                                      stream_of(topk_ids)));
}

// csrc/moe/moe_align_sum_kernels.cu (moe_sum): input [num_tokens, topk, hidden], output [num_tokens, hidden]
void moe_sum(const Tensor& input, Tensor& output) {
  need_devs(input, output);
  TORCH_CHECK(input.dim() == 3 && output.dim() == 2 && input.size(0) == output.size(0) &&
                  input.size(2) == output.size(1) && input.size(1) >= 1,
              "moe_sum: input [num_tokens, topk, hidden], output [num_tokens, hidden]");
  TORCH_CHECK(input.is_contiguous() && output.is_contiguous() && input.scalar_type() == output.scalar_type(),
              "moe_sum: contiguous tensors of one dtype required");
  DevGuard g(input.device());
  check(vllm_amd_moe_sum(output.data_ptr(), input.data_ptr(), input.size(0), (int)input.size(1), (int)input.size(2),
                         dt(input), stream_of(input)));
}

// The grouped GEMM of fused_experts (no reference op: its kernel is Triton, fused_moe.py:268-475).
// c [num_valid_tokens, N] or [tokens, top_k', N]; a [num_valid_tokens / top_k, K] fp8; b [E, N, K] fp8;
// a_scales [rows, K/128]; b_scales [E, ceil(N/128), K/128].
void moe_block_fp8_gemm(Tensor& c, const Tensor& a, const Tensor& b, const Tensor& a_scales, const Tensor& b_scales,
                        const OptTensor& topk_weights, const Tensor& sorted_token_ids, const Tensor& expert_ids,
                        const Tensor& num_tokens_post_padded, bool mul_routed_weight, int64_t top_k,
                        int64_t block_size_m) {
  need_devs(c, a, b, a_scales, b_scales, topk_weights, sorted_token_ids, expert_ids, num_tokens_post_padded);
  TORCH_CHECK(a.dim() == 2 && b.dim() == 3 && (c.dim() == 2 || c.dim() == 3) && a_scales.dim() == 2 &&
                  b_scales.dim() == 3,
              "moe_block_fp8_gemm: a [rows, K], b [E, N, K], c [rows * top_k, N], a_scales 2-D, b_scales 3-D");
  const int64_t K = a.size(1), E = b.size(0), N = b.size(1), kb = K / 128, nb = (N + 127) / 128;
  TORCH_CHECK(c.size(-1) == N && c.stride(-1) == 1 && (c.dim() == 2 || c.stride(0) == c.size(1) * c.stride(1)),
              "moe_block_fp8_gemm: c must have N contiguous columns and evenly strided rows");
  const int64_t nvt = N ? c.numel() / N : 0;
  TORCH_CHECK(top_k >= 1 && a.size(0) * top_k == nvt, "moe_block_fp8_gemm: c rows == a rows * top_k");
  TORCH_CHECK(b.size(2) == K && a.stride(1) == 1 && b.stride(2) == 1, "moe_block_fp8_gemm: K mismatch / K not contiguous");
  TORCH_CHECK(is_fp8(a) && is_fp8(b), "moe_block_fp8_gemm: fp8 e4m3 operands required");
  TORCH_CHECK(c.scalar_type() == at::kBFloat16 || c.scalar_type() == at::kHalf,
              "moe_block_fp8_gemm: c must be bfloat16 or float16, got ", c.scalar_type());
  TORCH_CHECK(a_scales.scalar_type() == at::kFloat && b_scales.scalar_type() == at::kFloat && a_scales.size(0) == a.size(0) &&
                  a_scales.size(1) == kb && b_scales.size(0) == E && b_scales.size(1) == nb && b_scales.size(2) == kb,
              "moe_block_fp8_gemm: float32 a_scales [rows, K/128] and b_scales [E, ceil(N/128), K/128] required");
  TORCH_CHECK(is_i32(sorted_token_ids) && is_i32(expert_ids) && is_i32(num_tokens_post_padded),
              "moe_block_fp8_gemm: contiguous int32 sorted_token_ids / expert_ids / num_tokens_post_padded required");
  TORCH_CHECK(block_size_m > 0, "moe_block_fp8_gemm: block_size_m > 0");
  // the grid and the cap of the device-side count come from the length of sorted_token_ids, as in the
  // reference's launch (fused_moe.py:519-528): with an expert_map it was aligned for the global expert
  // count; and as there, never more than one block per slot (every non-empty expert holds a slot)
  const int64_t max_padded = std::min<int64_t>(sorted_token_ids.numel(), nvt * block_size_m);
  TORCH_CHECK(sorted_token_ids.numel() >= nvt && max_padded < INT32_MAX &&
                  expert_ids.numel() >= (max_padded + block_size_m - 1) / block_size_m &&
                  num_tokens_post_padded.numel() >= 1,
              "moe_block_fp8_gemm: sorted_token_ids holds fewer entries than c has rows, or expert_ids fewer than one "
              "per block_size_m entries of it");
  TORCH_CHECK(!mul_routed_weight || topk_weights.has_value(), "moe_block_fp8_gemm: mul_routed_weight needs topk_weights");
  TORCH_CHECK(!topk_weights.has_value() || (topk_weights->scalar_type() == at::kFloat && topk_weights->is_contiguous() &&
                                            topk_weights->numel() == nvt),
              "moe_block_fp8_gemm: topk_weights must be contiguous float32 with one entry per row of c");
  DevGuard g(a.device());
  check(vllm_amd_moe_blockwise_gemm(
      c.data_ptr(), a.data_ptr(), b.data_ptr(), fptr(a_scales), fptr(b_scales),
      (const int32_t*)sorted_token_ids.data_ptr(), (const int32_t*)expert_ids.data_ptr(),
      (const int32_t*)num_tokens_post_padded.data_ptr(), fptr(topk_weights), (int)nvt, (int)top_k,
      mul_routed_weight ? 1 : 0, (int)block_size_m, (int)max_padded, (int)E, (int)N, (int)K, a.stride(0), b.stride(0), b.stride(1),
      c.stride(-2), a_scales.stride(0), a_scales.stride(1), b_scales.stride(0), b_scales.stride(1), b_scales.stride(2),
      dt(c), stream_of(a)));
}

// ---- MoE routing (csrc/moe_routing.hip) --------------------------------------------------------
// gating_output [tokens, experts] float32 / float16 / bfloat16 with contiguous experts; outputs [tokens, topk]
void route_check(const char* op, const Tensor& w, const Tensor& ids, const Tensor& gating) {
  TORCH_CHECK(gating.dim() == 2 && (gating.size(1) <= 1 || gating.stride(1) == 1) && is_16_32(gating), op,
              ": gating_output must be [num_tokens, num_experts] float32 / float16 / bfloat16 with contiguous experts");
  TORCH_CHECK(w.dim() == 2 && w.size(0) == gating.size(0) && w.scalar_type() == at::kFloat && w.is_contiguous(), op,
              ": topk_weights must be contiguous float32 [num_tokens, topk]");
  TORCH_CHECK(ids.sizes() == w.sizes() && ids.is_contiguous(), op, ": topk_ids must be contiguous [num_tokens, topk]");
}

// fused_topk's whole device work (fused_moe.py:882-915): softmax, top-k and, with `renormalize`, the division
void fused_topk(Tensor& topk_weights, Tensor& topk_ids, Tensor& token_expert_indices, const Tensor& gating_output,
                bool renormalize) {
  need_devs(topk_weights, topk_ids, token_expert_indices, gating_output);
  route_check("topk_softmax", topk_weights, topk_ids, gating_output);
  TORCH_CHECK(topk_ids.scalar_type() == at::kInt || topk_ids.scalar_type() == at::kLong,
              "topk_softmax: topk_indices must be int32 or int64, got ", topk_ids.scalar_type());
  TORCH_CHECK(is_i32(token_expert_indices) && token_expert_indices.sizes() == topk_weights.sizes(),
              "topk_softmax: token_expert_indices must be contiguous int32 [num_tokens, topk]");
  DevGuard g(gating_output.device());
  check(vllm_amd_topk_softmax((float*)topk_weights.data_ptr(), topk_ids.data_ptr(),
                              (int32_t*)token_expert_indices.data_ptr(), gating_output.data_ptr(), gating_output.size(0),
                              (int)gating_output.size(1), (int)topk_weights.size(1), gating_output.stride(0),
                              renormalize ? 1 : 0, dt(gating_output), topk_ids.scalar_type() == at::kLong ? 1 : 0,
                              stream_of(gating_output)));
}

// csrc/moe/topk_softmax_kernels.cu (topk_softmax)
void topk_softmax(Tensor& topk_weights, Tensor& topk_indices, Tensor& token_expert_indices, const Tensor& gating_output) {
  fused_topk(topk_weights, topk_indices, token_expert_indices, gating_output, false);
}

// the reference's torch grouped_topk (fused_moe.py:920-975) as one op
void grouped_topk(Tensor& topk_weights, Tensor& topk_ids, const Tensor& gating_output,
                  const OptTensor& e_score_correction_bias, int64_t num_expert_group, int64_t topk_group,
                  bool renormalize, const std::string& scoring_func) {
  need_devs(topk_weights, topk_ids, gating_output, e_score_correction_bias);
  route_check("grouped_topk", topk_weights, topk_ids, gating_output);
  TORCH_CHECK(is_i32(topk_ids), "grouped_topk: topk_ids must be int32, got ", topk_ids.scalar_type());
  TORCH_CHECK(scoring_func == "softmax" || scoring_func == "sigmoid", "Unsupported scoring function: ", scoring_func);
  TORCH_CHECK(!e_score_correction_bias.has_value() ||
                  (e_score_correction_bias->scalar_type() == at::kFloat && e_score_correction_bias->is_contiguous() &&
                   e_score_correction_bias->numel() == gating_output.size(1)),
              "grouped_topk: e_score_correction_bias must be contiguous float32 with one entry per expert");
  TORCH_CHECK(num_expert_group >= INT32_MIN && num_expert_group <= INT32_MAX && topk_group >= INT32_MIN &&
                  topk_group <= INT32_MAX, "grouped_topk: num_expert_group / topk_group out of range");
  DevGuard g(gating_output.device());
  check(vllm_amd_grouped_topk((float*)topk_weights.data_ptr(), (int32_t*)topk_ids.data_ptr(), gating_output.data_ptr(),
                              fptr(e_score_correction_bias), gating_output.size(0), (int)gating_output.size(1),
                              (int)topk_weights.size(1), (int)num_expert_group, (int)topk_group,
                              scoring_func == "sigmoid" ? VLLM_AMD_SCORE_SIGMOID : VLLM_AMD_SCORE_SOFTMAX,
                              renormalize ? 1 : 0, gating_output.stride(0), dt(gating_output), stream_of(gating_output)));
}

// silu_and_mul + per_token_group_fp8_quant (group 128) in one pass; input [rows, 2 d]
void silu_and_mul_group_quant(Tensor& output_q, Tensor& output_s, const Tensor& input) {
  need_devs(output_q, output_s, input);
  fp8_out(output_q);
  TORCH_CHECK(input.dim() == 2 && input.is_contiguous() && input.size(1) % 2 == 0,
              "silu_and_mul_group_quant: contiguous input [rows, 2 * d] required");
  const int64_t rows = input.size(0), d = input.size(1) / 2;
  TORCH_CHECK(input.scalar_type() == at::kBFloat16 || input.scalar_type() == at::kHalf,
              "silu_and_mul_group_quant: input must be bfloat16 or float16, got ", input.scalar_type());
  TORCH_CHECK(output_q.dim() == 2 && output_q.size(0) == rows && output_q.size(1) == d && output_s.dim() == 2 &&
                  output_s.scalar_type() == at::kFloat &&
                  output_s.size(0) == rows && output_s.size(1) == d / 128,
              "silu_and_mul_group_quant: output_q [rows, d], output_s float32 [rows, d / 128]");
  DevGuard g(input.device());
  check(vllm_amd_silu_and_mul_group_quant(output_q.data_ptr(), (float*)output_s.data_ptr(), input.data_ptr(), rows,
                                          (int)d, output_s.stride(0), output_s.stride(1), dt(input),
                                          stream_of(input)));
}

// ---- fused MoE over MXFP4 weights and activations (csrc/moe_mxfp4.hip) -----------------------------
inline bool is_u8(const Tensor& t) { return t.scalar_type() == at::kByte; }

// codes [rows, K / 2] and e8m0 scale bytes [rows, K / 32] of a 16-bit [rows, K]
void mxfp4_out_check(const char* op, const Tensor& q, const Tensor& s, int64_t rows, int64_t d) {
  TORCH_CHECK(d % 32 == 0, op, ": row length ", d, " is not a multiple of the 32-wide MX block");
  TORCH_CHECK(is_u8(q) && is_u8(s) && q.is_contiguous() && s.is_contiguous() && q.dim() == 2 && s.dim() == 2 &&
                  q.size(0) == rows && q.size(1) == d / 2 && s.size(0) == rows && s.size(1) == d / 32,
              op, ": contiguous uint8 output_q [rows, d / 2] and output_s [rows, d / 32] required");
}

void mxfp4_quant(Tensor& output_q, Tensor& output_s, const Tensor& input) {
  need_devs(output_q, output_s, input);
  TORCH_CHECK(input.dim() == 2 && (input.size(1) <= 1 || input.stride(1) == 1),
              "mxfp4_quant: input [rows, K] with K contiguous required");
  TORCH_CHECK(input.scalar_type() == at::kBFloat16 || input.scalar_type() == at::kHalf,
              "mxfp4_quant: input must be bfloat16 or float16, got ", input.scalar_type());
  mxfp4_out_check("mxfp4_quant", output_q, output_s, input.size(0), input.size(1));
  DevGuard g(input.device());
  check(vllm_amd_mxfp4_quant(output_q.data_ptr(), output_s.data_ptr(), input.data_ptr(), input.size(0),
                             (int)input.size(1), input.size(0) > 1 ? input.stride(0) : input.size(1), dt(input),
                             stream_of(input)));
}

// silu_and_mul + the MXFP4 quantiser in one pass; input [rows, 2 d]
void silu_and_mul_mxfp4_quant(Tensor& output_q, Tensor& output_s, const Tensor& input) {
  need_devs(output_q, output_s, input);
  TORCH_CHECK(input.dim() == 2 && input.is_contiguous() && input.size(1) % 2 == 0,
              "silu_and_mul_mxfp4_quant: contiguous input [rows, 2 * d] required");
  TORCH_CHECK(input.scalar_type() == at::kBFloat16 || input.scalar_type() == at::kHalf,
              "silu_and_mul_mxfp4_quant: input must be bfloat16 or float16, got ", input.scalar_type());
  mxfp4_out_check("silu_and_mul_mxfp4_quant", output_q, output_s, input.size(0), input.size(1) / 2);
  DevGuard g(input.device());
  check(vllm_amd_silu_and_mul_mxfp4_quant(output_q.data_ptr(), output_s.data_ptr(), input.data_ptr(), input.size(0),
                                          (int)(input.size(1) / 2), dt(input), stream_of(input)));
}

// The grouped GEMM of fused_experts(use_mxfp4_w4a4=True): the arguments of moe_block_fp8_gemm with
// a [rows, K / 2] and b [E, N, K / 2] uint8 codes, a_scales [rows, K / 32] and b_scales [E, N, K / 32] uint8 e8m0.
void moe_mxfp4_gemm(Tensor& c, const Tensor& a, const Tensor& b, const Tensor& a_scales, const Tensor& b_scales,
                    const OptTensor& topk_weights, const Tensor& sorted_token_ids, const Tensor& expert_ids,
                    const Tensor& num_tokens_post_padded, bool mul_routed_weight, int64_t top_k,
                    int64_t block_size_m) {
  need_devs(c, a, b, a_scales, b_scales, topk_weights, sorted_token_ids, expert_ids, num_tokens_post_padded);
  TORCH_CHECK(a.dim() == 2 && b.dim() == 3 && (c.dim() == 2 || c.dim() == 3) && a_scales.dim() == 2 &&
                  b_scales.dim() == 3,
              "moe_mxfp4_gemm: a [rows, K/2], b [E, N, K/2], c [rows * top_k, N], a_scales 2-D, b_scales 3-D");
  const int64_t K = a.size(1) * 2, E = b.size(0), N = b.size(1);
  TORCH_CHECK(c.size(-1) == N && c.stride(-1) == 1 && (c.dim() == 2 || c.stride(0) == c.size(1) * c.stride(1)),
              "moe_mxfp4_gemm: c must have N contiguous columns and evenly strided rows");
  const int64_t nvt = N ? c.numel() / N : 0;
  TORCH_CHECK(top_k >= 1 && a.size(0) * top_k == nvt, "moe_mxfp4_gemm: c rows == a rows * top_k");
  TORCH_CHECK(is_u8(a) && is_u8(b) && is_u8(a_scales) && is_u8(b_scales),
              "moe_mxfp4_gemm: uint8 codes and e8m0 scale bytes required");
  TORCH_CHECK(b.size(2) * 2 == K && a.stride(1) == 1 && b.stride(2) == 1 && a_scales.stride(1) == 1 &&
                  b_scales.stride(2) == 1,
              "moe_mxfp4_gemm: K mismatch / K not contiguous");
  TORCH_CHECK(c.scalar_type() == at::kBFloat16 || c.scalar_type() == at::kHalf,
              "moe_mxfp4_gemm: c must be bfloat16 or float16, got ", c.scalar_type());
  TORCH_CHECK(a_scales.size(0) == a.size(0) && a_scales.size(1) * 32 == K && b_scales.size(0) == E &&
                  b_scales.size(1) == N && b_scales.size(2) * 32 == K,
              "moe_mxfp4_gemm: a_scales [rows, K/32] and b_scales [E, N, K/32] required");
  TORCH_CHECK(is_i32(sorted_token_ids) && is_i32(expert_ids) && is_i32(num_tokens_post_padded),
              "moe_mxfp4_gemm: contiguous int32 sorted_token_ids / expert_ids / num_tokens_post_padded required");
  TORCH_CHECK(block_size_m > 0, "moe_mxfp4_gemm: block_size_m > 0");
  // the bound and its cap as in moe_block_fp8_gemm
  const int64_t max_padded = std::min<int64_t>(sorted_token_ids.numel(), nvt * block_size_m);
  TORCH_CHECK(sorted_token_ids.numel() >= nvt && max_padded < INT32_MAX &&
                  expert_ids.numel() >= (max_padded + block_size_m - 1) / block_size_m &&
                  num_tokens_post_padded.numel() >= 1,
              "moe_mxfp4_gemm: sorted_token_ids holds fewer entries than c has rows, or expert_ids fewer than one "
              "per block_size_m entries of it");
  TORCH_CHECK(!mul_routed_weight || topk_weights.has_value(), "moe_mxfp4_gemm: mul_routed_weight needs topk_weights");
  TORCH_CHECK(!topk_weights.has_value() || (topk_weights->scalar_type() == at::kFloat && topk_weights->is_contiguous() &&
                                            topk_weights->numel() == nvt),
              "moe_mxfp4_gemm: topk_weights must be contiguous float32 with one entry per row of c");
  DevGuard g(a.device());
  check(vllm_amd_moe_mxfp4_gemm(
      c.data_ptr(), a.data_ptr(), b.data_ptr(), a_scales.data_ptr(), b_scales.data_ptr(),
      (const int32_t*)sorted_token_ids.data_ptr(), (const int32_t*)expert_ids.data_ptr(),
      (const int32_t*)num_tokens_post_padded.data_ptr(), fptr(topk_weights), (int)nvt, (int)top_k,
      mul_routed_weight ? 1 : 0, (int)block_size_m, (int)max_padded, (int)E, (int)N, (int)K, a.stride(0), b.stride(0),
      b.stride(1), c.stride(-2), a_scales.stride(0), b_scales.stride(0), b_scales.stride(1), dt(c), stream_of(a)));
}

void wvSplitKQ(const Tensor& in_a, const Tensor& in_b, Tensor& out_c, const Tensor& scale_a, const Tensor& scale_b,
               int64_t cu_count) {
  need_devs(in_a, in_b, out_c, scale_a, scale_b);
  TORCH_CHECK(in_a.dim() == 2 && in_b.dim() == 2, "wvSplitKQ: 2-D operands required");
  TORCH_CHECK(in_a.is_contiguous() && in_b.is_contiguous() && out_c.is_contiguous(),
              "wvSplitKQ: contiguous tensors required");
  TORCH_CHECK(in_b.size(1) == in_a.size(1), "in_a.size(1) == in_b.size(1)");
  DevGuard g(in_a.device());
  check(vllm_amd_wvSplitKQ(in_a.data_ptr(), in_b.data_ptr(), out_c.data_ptr(), fptr(scale_a), fptr(scale_b),
                           (int)in_a.size(0), (int)in_a.size(1), (int)in_b.size(0), dt(out_c), (int)cu_count,
                           stream_of(in_a)));
}

// ---- fused neighbours -------------------------------------------------------
// csrc/layernorm_quant_kernels.cu:172-198
void rms_norm_static_fp8_quant(Tensor& result, const Tensor& input, const Tensor& weight, const Tensor& scale,
                               double epsilon) {
  need_devs(result, input, weight, scale);
  fp8_out(result);
  const int64_t hidden = input.size(-1);
  DevGuard g(input.device());
  check(vllm_amd_rms_norm_static_fp8_quant(result.data_ptr(), input.data_ptr(), weight.data_ptr(), fptr(scale),
                                           (float)epsilon, rows_of(input, hidden), (int)hidden,
                                           input.dim() >= 2 ? input.stride(-2) : hidden, dt(input),
                                           stream_of(input)));
}

// csrc/layernorm_quant_kernels.cu:214-253
void fused_add_rms_norm_static_fp8_quant(Tensor& result, const Tensor& input, Tensor& residual,
                                         const Tensor& weight, const Tensor& scale, double epsilon) {
  need_devs(result, input, residual, weight, scale);
  fp8_out(result);
  TORCH_CHECK(residual.is_contiguous(), "residual.is_contiguous()");
  const int64_t hidden = input.size(-1);
  DevGuard g(input.device());
  check(vllm_amd_fused_add_rms_norm_static_fp8_quant(
      result.data_ptr(), input.data_ptr(), residual.data_ptr(), weight.data_ptr(), fptr(scale), (float)epsilon,
      rows_of(input, hidden), (int)hidden, input.dim() >= 2 ? input.stride(-2) : hidden, dt(input),
      stream_of(input)));
}

// csrc/quantization/fused_kernels/fused_layernorm_dynamic_per_token_quant.cu:132-155
void rms_norm_dynamic_per_token_quant(Tensor& result, const Tensor& input, const Tensor& weight, Tensor& scale,
                                      double epsilon, const OptTensor& scale_ub, OptTensor residual) {
  need_devs(result, input, weight, scale, scale_ub, residual);
  const bool i8 = result.scalar_type() == at::kChar;
  if (i8) {
    // fused_layernorm_dynamic_per_token_quant.cu:139-146: int8 or fp8 output, scale_ub only with fp8
    TORCH_CHECK(!scale_ub.has_value(), "rms_norm_dynamic_per_token_quant: scale_ub needs an fp8 output");
    TORCH_CHECK(result.is_contiguous(), "out.is_contiguous()");
  } else {
    fp8_out(result);
  }
  TORCH_CHECK(input.is_contiguous(), "input.is_contiguous()");
  TORCH_CHECK(scale.scalar_type() == at::kFloat, "scales.dtype() == torch::kFloat32");
  TORCH_CHECK(!residual.has_value() || residual->is_contiguous(), "residual.is_contiguous()");
  const int64_t hidden = input.size(-1);
  DevGuard g(input.device());
  if (i8)
    check(vllm_amd_rms_norm_dynamic_per_token_quant_int8(result.data_ptr(), input.data_ptr(), weight.data_ptr(),
                                                         (float*)scale.data_ptr(), (float)epsilon, vptr(residual),
                                                         rows_of(input, hidden), (int)hidden, dt(input),
                                                         stream_of(input)));
  else
    check(vllm_amd_rms_norm_dynamic_per_token_quant(result.data_ptr(), input.data_ptr(), weight.data_ptr(),
                                                    (float*)scale.data_ptr(), (float)epsilon, fptr(scale_ub),
                                                    vptr(residual), rows_of(input, hidden), (int)hidden, dt(input),
                                                    stream_of(input)));
}

// csrc/quantization/activation_kernels.cu:112-121
void silu_and_mul_quant(Tensor& result, const Tensor& input, const Tensor& scale) {
  need_devs(result, input, scale);
  fp8_out(result);
  TORCH_CHECK(input.scalar_type() == at::kHalf || input.scalar_type() == at::kBFloat16,
              "input.dtype() == torch::kFloat16 || input.dtype() == torch::kBFloat16");
  TORCH_CHECK(input.size(-1) % 2 == 0, "input.size(-1) % 2 == 0");
  TORCH_CHECK(input.is_contiguous(), "input.is_contiguous()");
  const int64_t d = input.size(-1) / 2;
  DevGuard g(input.device());
  check(vllm_amd_silu_and_mul_quant(result.data_ptr(), input.data_ptr(), fptr(scale),
                                    d ? input.numel() / input.size(-1) : 0, (int)d, dt(input), stream_of(input)));
}

// Device-side BlockTable.compute_slot_mapping (vllm/v1/worker/block_table.py:84-99).  Not a
// reference op (the reference does this with numpy on the host): namespace _vllm_amd_C.
void compute_slot_mapping(Tensor& slot_mapping, const Tensor& block_table, const Tensor& req_indices,
                          const Tensor& positions, int64_t block_size) {
  need_devs(slot_mapping, block_table, req_indices, positions);
  TORCH_CHECK(slot_mapping.scalar_type() == at::kLong && positions.scalar_type() == at::kLong &&
                  block_table.scalar_type() == at::kInt && req_indices.scalar_type() == at::kInt,
              "compute_slot_mapping: slot_mapping / positions int64, block_table / req_indices int32");
  TORCH_CHECK(block_table.dim() == 2 && block_table.is_contiguous() && req_indices.is_contiguous() &&
                  positions.is_contiguous() && slot_mapping.is_contiguous(),
              "compute_slot_mapping: contiguous tensors required");
  const int64_t n = req_indices.size(0);
  TORCH_CHECK(slot_mapping.size(0) >= n && positions.size(0) >= n, "compute_slot_mapping: outputs shorter than n");
  DevGuard g(block_table.device());
  check(vllm_amd_compute_slot_mapping((int64_t*)slot_mapping.data_ptr(), (const int32_t*)block_table.data_ptr(),
                                      (const int32_t*)req_indices.data_ptr(), (const int64_t*)positions.data_ptr(),
                                      n, (int)block_table.size(1), (int)block_size, stream_of(block_table)));
}

// ---- registration ------------------------------------------------------------------------
#define PA_TAIL                                                                                               \
  " int num_kv_heads, float scale, Tensor block_tables, Tensor seq_lens, int block_size,"                   \
  " int max_seq_len, Tensor? alibi_slopes, str kv_cache_dtype, Tensor k_scale,"                              \
  " Tensor v_scale, int tp_rank, int blocksparse_local_blocks,"                                              \
  " int blocksparse_vert_stride, int blocksparse_block_size,"                                                \
  " int blocksparse_head_sliding_step) -> ()"

std::vector<std::unique_ptr<torch::Library>> g_libs;   // kept alive for the life of the process

struct Registrar {
  const char* ns;
  torch::Library* frag;
  torch::Library* impl;
  torch::Library* impl_any;
  template <class F>
  void op(const char* name, const char* schema, F* fn, bool any_device = false) {
    try {
      frag->def(schema);
    } catch (const c10::Error&) {
      // already defined (the real vLLM extension was imported first): override the kernel only
    }
    (any_device ? impl_any : impl)->impl(name, fn);
  }
};

Registrar open_ns(const char* ns) {
  auto mk = [&](torch::Library::Kind kind, std::optional<c10::DispatchKey> k) {
    g_libs.emplace_back(new torch::Library(kind, ns, k, __FILE__, __LINE__));
    return g_libs.back().get();
  };
  return Registrar{ns, mk(torch::Library::FRAGMENT, std::nullopt),
                   mk(torch::Library::IMPL, c10::DispatchKey::CUDA),
                   mk(torch::Library::IMPL, c10::DispatchKey::CompositeExplicitAutograd)};
}

void register_all() {
  Registrar c = open_ns("_C");
  c.op("paged_attention_v1",
       "paged_attention_v1(Tensor! out, Tensor query, Tensor key_cache, Tensor value_cache," PA_TAIL,
       &paged_attention_v1);
  c.op("paged_attention_v2",
       "paged_attention_v2(Tensor! out, Tensor! exp_sums, Tensor! max_logits, Tensor! tmp_out,"
       " Tensor query, Tensor key_cache, Tensor value_cache," PA_TAIL,
       &paged_attention_v2);
  c.op("static_scaled_fp8_quant", "static_scaled_fp8_quant(Tensor! result, Tensor input, Tensor scale) -> ()",
       &static_scaled_fp8_quant);
  c.op("dynamic_scaled_fp8_quant", "dynamic_scaled_fp8_quant(Tensor! result, Tensor input, Tensor! scale) -> ()",
       &dynamic_scaled_fp8_quant);
  c.op("dynamic_per_token_scaled_fp8_quant",
       "dynamic_per_token_scaled_fp8_quant(Tensor! result, Tensor input, Tensor! scale,"
       " Tensor? scale_ub) -> ()",
       &dynamic_per_token_scaled_fp8_quant);
  c.op("per_token_group_fp8_quant",
       "per_token_group_fp8_quant(Tensor input, Tensor! output_q, Tensor! output_s, "
       "int group_size, float eps, float fp8_min, float fp8_max, bool scale_ue8m0) -> ()",
       &per_token_group_fp8_quant);
  c.op("cutlass_scaled_mm",
       "cutlass_scaled_mm(Tensor! out, Tensor a, Tensor b, Tensor a_scales, Tensor b_scales,"
       " Tensor? bias) -> ()",
       &cutlass_scaled_mm);
  c.op("silu_and_mul_quant", "silu_and_mul_quant(Tensor! result, Tensor input, Tensor scale) -> ()",
       &silu_and_mul_quant);
  c.op("rms_norm_static_fp8_quant",
       "rms_norm_static_fp8_quant(Tensor! result, Tensor input, Tensor weight, Tensor scale,"
       " float epsilon) -> ()",
       &rms_norm_static_fp8_quant);
  c.op("fused_add_rms_norm_static_fp8_quant",
       "fused_add_rms_norm_static_fp8_quant(Tensor! result, Tensor input, Tensor! residual,"
       " Tensor weight, Tensor scale, float epsilon) -> ()",
       &fused_add_rms_norm_static_fp8_quant);
  c.op("rms_norm_dynamic_per_token_quant",
       "rms_norm_dynamic_per_token_quant(Tensor! result, Tensor input, Tensor weight,"
       " Tensor! scale, float epsilon, Tensor? scale_ub, Tensor!? residual) -> ()",
       &rms_norm_dynamic_per_token_quant);

  // no reference counterpart (its grouped GEMM is Triton, its activation and quantiser two ops)
  c.op("moe_block_fp8_gemm",
       "moe_block_fp8_gemm(Tensor! c, Tensor a, Tensor b, Tensor a_scales, Tensor b_scales,"
       " Tensor? topk_weights, Tensor sorted_token_ids, Tensor expert_ids,"
       " Tensor num_tokens_post_padded, bool mul_routed_weight, int top_k, int block_size_m) -> ()",
       &moe_block_fp8_gemm);
  c.op("silu_and_mul_group_quant",
       "silu_and_mul_group_quant(Tensor! output_q, Tensor! output_s, Tensor input) -> ()",
       &silu_and_mul_group_quant);
  // the MXFP4 (w4a4) path: no reference counterparts either (there the weights are dequantised to bf16)
  c.op("mxfp4_quant", "mxfp4_quant(Tensor! output_q, Tensor! output_s, Tensor input) -> ()", &mxfp4_quant);
  c.op("silu_and_mul_mxfp4_quant",
       "silu_and_mul_mxfp4_quant(Tensor! output_q, Tensor! output_s, Tensor input) -> ()",
       &silu_and_mul_mxfp4_quant);
  c.op("moe_mxfp4_gemm",
       "moe_mxfp4_gemm(Tensor! c, Tensor a, Tensor b, Tensor a_scales, Tensor b_scales,"
       " Tensor? topk_weights, Tensor sorted_token_ids, Tensor expert_ids,"
       " Tensor num_tokens_post_padded, bool mul_routed_weight, int top_k, int block_size_m) -> ()",
       &moe_mxfp4_gemm);

  // csrc/moe/torch_bindings.cpp:13-22
  Registrar mo = open_ns("_moe_C");
  mo.op("moe_sum", "moe_sum(Tensor input, Tensor! output) -> ()", &moe_sum);
  mo.op("moe_align_block_size",
        "moe_align_block_size(Tensor topk_ids, int num_experts,"
        "                     int block_size, Tensor! sorted_token_ids,"
        "                     Tensor! experts_ids,"
        "                     Tensor! num_tokens_post_pad) -> ()",
        &moe_align_block_size);
  // csrc/moe/torch_bindings.cpp:6-9
  mo.op("topk_softmax",
        "topk_softmax(Tensor! topk_weights, Tensor! topk_indices, Tensor! "
        "token_expert_indices, Tensor gating_output) -> ()",
        &topk_softmax);
  // no reference counterparts: fused_topk renormalises in torch after its op, grouped_topk is torch code there
  mo.op("fused_topk",
        "fused_topk(Tensor! topk_weights, Tensor! topk_ids, Tensor! token_expert_indices, Tensor gating_output,"
        " bool renormalize) -> ()",
        &fused_topk);
  mo.op("grouped_topk",
        "grouped_topk(Tensor! topk_weights, Tensor! topk_ids, Tensor gating_output,"
        " Tensor? e_score_correction_bias, int num_expert_group, int topk_group, bool renormalize,"
        " str scoring_func) -> ()",
        &grouped_topk);

  Registrar k = open_ns("_C_cache_ops");
  k.op("reshape_and_cache",
       "reshape_and_cache(Tensor key, Tensor value, Tensor! key_cache, Tensor! value_cache,"
       " Tensor slot_mapping, str kv_cache_dtype, Tensor k_scale, Tensor v_scale) -> ()",
       &reshape_and_cache);
  k.op("reshape_and_cache_flash",
       "reshape_and_cache_flash(Tensor key, Tensor value, Tensor! key_cache,"
       " Tensor! value_cache, Tensor slot_mapping, str kv_cache_dtype, Tensor k_scale,"
       " Tensor v_scale) -> ()",
       &reshape_and_cache_flash);
  k.op("concat_and_cache_mla",
       "concat_and_cache_mla(Tensor kv_c, Tensor k_pe, Tensor! kv_cache, Tensor slot_mapping,"
       " str kv_cache_dtype, Tensor scale) -> ()",
       &concat_and_cache_mla);
  k.op("convert_fp8", "convert_fp8(Tensor! dst_cache, Tensor src_cache, float scale, str kv_cache_dtype) -> ()",
       &convert_fp8);
  // csrc/torch_bindings.cpp:710-714
  k.op("gather_cache",
       "gather_cache(Tensor src_cache, Tensor! dst, Tensor block_table, "
       "Tensor cu_seq_lens, int batch_size, Tensor? seq_starts) -> ()",
       &gather_cache);
  k.op("copy_blocks",
       "copy_blocks(Tensor(a!)[] key_caches, Tensor[](b!) value_caches,"
       " Tensor block_mapping) -> ()",
       &copy_blocks);
  k.op("swap_blocks", "swap_blocks(Tensor src, Tensor! dst, Tensor block_mapping) -> ()", &swap_blocks,
       /*any_device=*/true);

  Registrar r = open_ns("_rocm_C");
  r.op("paged_attention",
       "paged_attention(Tensor! out, Tensor exp_sums, Tensor max_logits, Tensor tmp_out,"
       " Tensor query, Tensor key_cache, Tensor value_cache, int num_kv_heads, float scale,"
       " Tensor block_tables, Tensor context_lens, Tensor? query_start_loc, int block_size,"
       " int max_context_len, Tensor? alibi_slopes, str kv_cache_dtype, Tensor k_scale,"
       " Tensor v_scale, Tensor? fp8_out_scale) -> ()",
       &paged_attention_rocm);
  r.op("wvSplitKQ",
       "wvSplitKQ(Tensor in_a, Tensor in_b, Tensor! out_c, Tensor scale_a, Tensor scale_b,"
       " int CuCount) -> ()",
       &wvSplitKQ);

  Registrar x = open_ns("_vllm_amd_C");
  x.op("compute_slot_mapping",
       "compute_slot_mapping(Tensor! slot_mapping, Tensor block_table, Tensor req_indices,"
       " Tensor positions, int block_size) -> ()",
       &compute_slot_mapping);
}

std::string g_reg_error;
bool g_registered = false;

}  // namespace

// Called once by vllm_amd/_torch_ops.py after dlopen (in tree: by whatever loads the plugin).
// Returns 0, or -1 with vllm_amd_torch_register_error() holding the message.
extern "C" int vllm_amd_torch_register(void) {
  if (g_registered) return 0;
  try {
    register_all();
    g_registered = true;
    return 0;
  } catch (const std::exception& e) {
    g_reg_error = e.what();
    return -1;
  }
}

extern "C" const char* vllm_amd_torch_register_error(void) { return g_reg_error.c_str(); }
