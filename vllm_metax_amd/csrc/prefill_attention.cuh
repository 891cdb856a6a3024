// prefill_attention.cuh — what the MFMA prefill kernels share (prefill_attention.hip: head size 128;
// prefill_attention_hd.hip: head sizes 64 and 256): the 16x16x32 MFMA wrappers with the exact fp8 -> 16-bit
// conversions, the in-register reductions over a wave's four 16-lane rows, and the host-side route note.
#pragma once

#include "common.cuh"

namespace mi355x {

template <typename T>
struct MfmaQK;
template <>
struct MfmaQK<bf16_t> {
  static __device__ __forceinline__ f32x4_t run(const uint4& a, const uint4& b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a),
                                                   __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ uint32_t pack(float lo, float hi) {
    bf16x2_t v = {static_cast<bf16_t>(lo), static_cast<bf16_t>(hi)};
    return __builtin_bit_cast(uint32_t, v);
  }
  // 4 e4m3 (E5M2: e5m2) bytes -> 4 bf16 (two packed words), exact
  template <bool E5M2 = false>
  static __device__ __forceinline__ uint2 from_fp8x4(uint32_t w) {
    if constexpr (E5M2)
      return make_uint2(
          __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_bf8(w, 1.0f, false)),
          __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_bf8(w, 1.0f, true)));
    else
      return make_uint2(
          __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false)),
          __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true)));
  }
};
template <>
struct MfmaQK<f16_t> {
  static __device__ __forceinline__ f32x4_t run(const uint4& a, const uint4& b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a),
                                                  __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ uint32_t pack(float lo, float hi) {
    f16x2_t v = {static_cast<f16_t>(lo), static_cast<f16_t>(hi)};
    return __builtin_bit_cast(uint32_t, v);
  }
  template <bool E5M2 = false>
  static __device__ __forceinline__ uint2 from_fp8x4(uint32_t w) {
    if constexpr (E5M2)
      return make_uint2(
          __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_bf8(w, 1.0f, false)),
          __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_bf8(w, 1.0f, true)));
    else
      return make_uint2(
          __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, false)),
          __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, true)));
  }
};

// all-reduce over the four 16-lane rows of a wave (lanes l, l ^ 16, l ^ 32, l ^ 48) in registers: gfx950's
// v_permlane16_swap / v_permlane32_swap exchange row pairs / wave halves (vdst's odd rows with src's even rows;
// vdst's upper half with src's lower half), so op(swap(x, x)) is the xor-16 / xor-32 butterfly step without the
// LDS round trip of ds_bpermute (__shfl_xor).
__device__ __forceinline__ float rows_max(float x) {
  const uint32_t u = __builtin_bit_cast(uint32_t, x);
  auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  x = fmaxf(__builtin_bit_cast(float, (uint32_t)r[0]), __builtin_bit_cast(float, (uint32_t)r[1]));
  const uint32_t v = __builtin_bit_cast(uint32_t, x);
  auto q = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  return fmaxf(__builtin_bit_cast(float, (uint32_t)q[0]), __builtin_bit_cast(float, (uint32_t)q[1]));
}
__device__ __forceinline__ float rows_sum(float x) {
  const uint32_t u = __builtin_bit_cast(uint32_t, x);
  auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  x = __builtin_bit_cast(float, (uint32_t)r[0]) + __builtin_bit_cast(float, (uint32_t)r[1]);
  const uint32_t v = __builtin_bit_cast(uint32_t, x);
  auto q = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  return __builtin_bit_cast(float, (uint32_t)q[0]) + __builtin_bit_cast(float, (uint32_t)q[1]);
}

constexpr float kNegBig = -1.0e30f;

// mi355x_paged_prefill_last_route: the kernel the current prefill entry launched (MI355X_PF_ROUTE_*; defined in
// prefill_attention.hip).  Host-side bookkeeping only: every entry clears it, the launch site sets it.
extern thread_local int pf_route;

// Arguments of one prefill call, as the C entry points receive them (prefill_attention.hip validates them).
struct PrefillArgs {
  void* out;
  const void *query, *key_cache, *value_cache;
  int num_seqs, num_heads, num_kv_heads, head_size;
  float scale;
  const int *block_tables, *seq_lens, *cu_seqlens_q;
  int max_query_len, max_num_blocks_per_seq;
  int64_t q_stride, out_stride, kv_block_stride, kv_head_stride;
  int dtype, kv_cache_dtype;
  const float *k_scale, *v_scale;
  int sliding_window;
  float softcap;
  hipStream_t stream;
};
// head_size 64 / 256, block_size 16, 16-bit dtype, aligned operands (the caller has checked): launches
// paged_prefill_hd_kernel (prefill_attention_hd.hip)
int paged_prefill_hd_launch(const PrefillArgs& a);

}  // namespace mi355x
