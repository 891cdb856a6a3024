// fp8_quant.hip — activation -> float8_e4m3fn quantisation for gfx950.
//
// Reference semantics restated (csrc/quantization/fp8/common.cu:11-133,
// common.cuh:25-38, quantization/utils.cuh:15-44):
//   static :  q = sat( float(x) * (1/scale) )
//   dynamic:  scale = max over tensor of absmax(row)/448, folded with an atomic max
//             into a caller-zeroed scalar; then q = sat( float(x) * (1/scale) )
//   per-tok:  s = max( min(absmax, ub)/448, 1/(448*512) ); q = sat( float(x) / s )
//   per-tok-group (128): s = max(absmax of the group, eps)/448; q = sat( float(x) / s )  (block-scaled GEMM input)
//   per-tok-group, UE8M0 (128 | 32): s = 2^ceil(log2(max(absmax, eps)/448)); q = sat( float(x) / s ), s as byte or float
// sat() clamps to +-448 and converts RNE (v_cvt_pk_fp8_f32, OCP e4m3fn on gfx950).
// One workgroup per token row, 16-B loads / 8-B stores when the row is aligned.
#include "common.cuh"

namespace mi355x {

template <typename T, bool VEC, typename F>
__device__ __forceinline__ void for_each_row_elem(const T* row, int n, F&& f) {
  if constexpr (VEC) {
    constexpr int V = 16 / sizeof(T);
    for (int i = threadIdx.x * V; i < n; i += blockDim.x * V) {
      T v[V];
      *reinterpret_cast<uint4*>(v) = *reinterpret_cast<const uint4*>(row + i);
#pragma unroll
      for (int j = 0; j < V; ++j) f(i + j, to_f32(v[j]));
    }
  } else {
    for (int i = threadIdx.x; i < n; i += blockDim.x) f(i, to_f32(row[i]));
  }
}

template <typename T, bool VEC, bool DIVIDE>
__device__ __forceinline__ void quant_row(uint8_t* out_row, const T* row, int n, float s) {
  RowDiv rdiv{};
  if constexpr (DIVIDE) rdiv = make_row_div(s);   // x / s, the bits of the division (common.cuh)
  if constexpr (VEC) {
    constexpr int V = 16 / sizeof(T);
    for (int i = threadIdx.x * V; i < n; i += blockDim.x * V) {
      T v[V];
      float y[V];
      *reinterpret_cast<uint4*>(v) = *reinterpret_cast<const uint4*>(row + i);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float x = to_f32(v[j]);
        if constexpr (DIVIDE) y[j] = row_div(x, rdiv);
        else y[j] = x * s;
      }
      if constexpr (V == 8) {
        *reinterpret_cast<uint2*>(out_row + i) = f32x8_to_fp8x8_sat(y);
      } else {
        *reinterpret_cast<uint32_t*>(out_row + i) = f32x4_to_fp8x4_sat(y);
      }
    }
  } else {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const float x = to_f32(row[i]);
      float y;
      if constexpr (DIVIDE) y = row_div(x, rdiv);
      else y = x * s;
      out_row[i] = f32_to_fp8_sat(y);
    }
  }
}

// static and dynamic-per-tensor second pass: multiply by 1/scale
template <typename T, bool VEC>
__global__ void scaled_fp8_quant_kernel(uint8_t* __restrict__ out, const T* __restrict__ in,
                                        const float* __restrict__ scale, int hidden,
                                        int64_t in_stride, int64_t out_stride) {
  const int64_t row = blockIdx.x;
  const float inv = 1.0f / *scale;
  quant_row<T, VEC, false>(out + row * out_stride, in + row * in_stride, hidden, inv);
}

template <typename T, bool VEC>
__global__ void absmax_to_scale_kernel(float* __restrict__ scale, const T* __restrict__ in,
                                       int hidden, int64_t in_stride) {
  __shared__ float red[16];
  const int64_t row = blockIdx.x;
  float m = 0.f;
  for_each_row_elem<T, VEC>(in + row * in_stride, hidden,
                            [&](int, float v) { m = fmaxf(m, fabsf(v)); });
  m = block_reduce<true>(m, red);
  if (threadIdx.x == 0) {
    // non-negative floats order like their bit patterns
    atomicMax(reinterpret_cast<int*>(scale), __float_as_int(m / kFp8Max));
  }
}

template <typename T, bool VEC>
__global__ void per_token_fp8_quant_kernel(uint8_t* __restrict__ out,
                                           float* __restrict__ scales,
                                           const T* __restrict__ in,
                                           const float* __restrict__ scale_ub, int hidden,
                                           int64_t in_stride, int64_t out_stride) {
  __shared__ float red[16];
  __shared__ float s_scale;
  const int64_t row = blockIdx.x;
  const T* rin = in + row * in_stride;
  float m = 0.f;
  for_each_row_elem<T, VEC>(rin, hidden, [&](int, float v) { m = fmaxf(m, fabsf(v)); });
  m = block_reduce<true>(m, red);
  if (threadIdx.x == 0) {
    float s = scale_ub ? fminf(m, *scale_ub) : m;
    s = fmaxf(s / kFp8Max, kFp8MinScale);
    scales[row] = s;
    s_scale = s;
  }
  __syncthreads();
  quant_row<T, VEC, true>(out + row * out_stride, rin, hidden, s_scale);
}

// per token and 128-wide group: s = max(absmax, eps) / 448, q = sat(x / s) — the activation side of the block-scaled
// GEMM (fp8_block_gemm.hip).  One workgroup per token, 16 bytes = 8 elements per lane, so a group is 16 adjacent lanes
// of one wave: its absmax is four butterfly steps, no LDS.  The division is the exact three-operation row division of
// the per-token kernel (common.cuh), with the group's scale as the divisor.
template <typename T>
__global__ void per_token_group_fp8_quant_kernel(uint8_t* __restrict__ out, float* __restrict__ scales,
                                                 const T* __restrict__ in, int hidden, int64_t in_stride,
                                                 int64_t out_stride, int64_t scale_row_stride,
                                                 int64_t scale_group_stride, float eps) {
  static_assert(sizeof(T) == 2, "8 elements per 16-byte load");
  const int64_t row = blockIdx.x;
  const T* rin = in + row * in_stride;
  for (int i = threadIdx.x * 8; i < hidden; i += blockDim.x * 8) {   // (whole groups: hidden % 128 == 0)
    T v[8];
    float x[8], y[8];
    *reinterpret_cast<uint4*>(v) = *reinterpret_cast<const uint4*>(rin + i);
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      x[j] = to_f32(v[j]);
      amax = fmaxf(amax, fabsf(x[j]));
    }
#pragma unroll
    for (int mask = 8; mask >= 1; mask >>= 1) amax = fmaxf(amax, __shfl_xor(amax, mask, 64));
    const float s = fmaxf(amax, eps) / kFp8Max;
    if ((threadIdx.x & 15) == 0) scales[row * scale_row_stride + (i >> 7) * scale_group_stride] = s;
    const RowDiv rdiv = make_row_div(s);
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = row_div(x[j], rdiv);
    *reinterpret_cast<uint2*>(out + row * out_stride + i) = f32x8_to_fp8x8_sat(y);
  }
}

// the same launch with power-of-two (UE8M0) scales — the activation side of fp8_e8m0_gemm.hip.  A group is GL = 16
// (128 wide) or 4 (32 wide) adjacent lanes.  s0 = max(absmax, eps) / 448 as above, rounded UP to a power of two:
// byte = exponent field + (mantissa != 0), at most 254, so |x| / 2^(byte - 127) <= 448; x * 2^(127 - byte) is exact,
// the conversion its only rounding.  S = uint8_t stores the byte, S = float the value 2^(byte - 127).
template <typename T, typename S, int GL>
__global__ void per_token_group_fp8_quant_ue8m0_kernel(uint8_t* __restrict__ out, S* __restrict__ scales,
                                                       const T* __restrict__ in, int hidden, int64_t in_stride,
                                                       int64_t out_stride, int64_t scale_row_stride,
                                                       int64_t scale_group_stride, float eps) {
  static_assert(sizeof(T) == 2, "8 elements per 16-byte load");
  const int64_t row = blockIdx.x;
  const T* rin = in + row * in_stride;
  for (int i = threadIdx.x * 8; i < hidden; i += blockDim.x * 8) {   // (whole groups: hidden % (8 GL) == 0)
    T v[8];
    float x[8], y[8];
    *reinterpret_cast<uint4*>(v) = *reinterpret_cast<const uint4*>(rin + i);
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      x[j] = to_f32(v[j]);
      amax = fmaxf(amax, fabsf(x[j]));
    }
#pragma unroll
    for (int mask = GL / 2; mask >= 1; mask >>= 1) amax = fmaxf(amax, __shfl_xor(amax, mask, 64));
    const uint32_t bits = __float_as_uint(fmaxf(amax, eps) / kFp8Max);
    const int byte = min((int)(bits >> 23) + ((bits & 0x7FFFFFu) != 0), 254);
    if ((threadIdx.x & (GL - 1)) == 0) {
      S* dst = scales + row * scale_row_stride + (i / (8 * GL)) * scale_group_stride;
      if constexpr (sizeof(S) == 1) *dst = (uint8_t)byte;
      else *dst = __uint_as_float(byte ? (uint32_t)byte << 23 : 0x00400000u);   // (2^-127 is subnormal)
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = __builtin_ldexpf(x[j], 127 - byte);
    *reinterpret_cast<uint2*>(out + row * out_stride + i) = f32x8_to_fp8x8_sat(y);
  }
}

template <typename T>
static bool row_vec_ok(const void* in, const void* out, int hidden, int64_t in_stride,
                       int64_t out_stride) {
  constexpr int V = 16 / sizeof(T);
  return hidden % V == 0 && in_stride % V == 0 && out_stride % V == 0 &&
         (reinterpret_cast<uintptr_t>(in) & 15) == 0 &&
         (reinterpret_cast<uintptr_t>(out) % V) == 0;
}

static int row_threads(int hidden, int per_thread) {
  int t = (hidden + per_thread - 1) / per_thread;
  t = ((t + 63) / 64) * 64;
  return t > 256 ? 256 : t;
}

}  // namespace mi355x

using namespace mi355x;

extern "C" {

int mi355x_static_scaled_fp8_quant(void* out, const void* input, const float* scale,
                                   int num_tokens, int hidden_size,
                                   int64_t in_row_stride, int64_t out_row_stride,
                                   int dtype, mi355x_stream stream) {
  MI355X_REQUIRE(num_tokens >= 0 && hidden_size > 0, MI355X_EINVAL,
                 "static_scaled_fp8_quant: bad sizes");
  if (num_tokens == 0) return MI355X_OK;
  MI355X_REQUIRE(out && input && scale, MI355X_EINVAL, "static_scaled_fp8_quant: null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  return MI355X_DISPATCH_FLOAT(dtype, [&] {
    const scalar_t* in = static_cast<const scalar_t*>(input);
    uint8_t* o = static_cast<uint8_t*>(out);
    const bool vec = row_vec_ok<scalar_t>(in, o, hidden_size, in_row_stride, out_row_stride);
    dim3 grid(num_tokens), block(row_threads(hidden_size, vec ? 16 / sizeof(scalar_t) : 1));
    if (vec)
      hipLaunchKernelGGL((scaled_fp8_quant_kernel<scalar_t, true>), grid, block, 0, s, o, in,
                         scale, hidden_size, in_row_stride, out_row_stride);
    else
      hipLaunchKernelGGL((scaled_fp8_quant_kernel<scalar_t, false>), grid, block, 0, s, o, in,
                         scale, hidden_size, in_row_stride, out_row_stride);
    return check_launch("static_scaled_fp8_quant");
  });
}

int mi355x_dynamic_scaled_fp8_quant(void* out, const void* input, float* scale,
                                    int num_tokens, int hidden_size,
                                    int64_t in_row_stride, int64_t out_row_stride,
                                    int dtype, mi355x_stream stream) {
  MI355X_REQUIRE(num_tokens >= 0 && hidden_size > 0, MI355X_EINVAL,
                 "dynamic_scaled_fp8_quant: bad sizes");
  if (num_tokens == 0) return MI355X_OK;
  MI355X_REQUIRE(out && input && scale, MI355X_EINVAL, "dynamic_scaled_fp8_quant: null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  return MI355X_DISPATCH_FLOAT(dtype, [&] {
    const scalar_t* in = static_cast<const scalar_t*>(input);
    uint8_t* o = static_cast<uint8_t*>(out);
    const bool vec = row_vec_ok<scalar_t>(in, o, hidden_size, in_row_stride, out_row_stride);
    dim3 grid(num_tokens), block(row_threads(hidden_size, vec ? 16 / sizeof(scalar_t) : 1));
    if (vec) {
      hipLaunchKernelGGL((absmax_to_scale_kernel<scalar_t, true>), grid, block, 0, s, scale, in,
                         hidden_size, in_row_stride);
      hipLaunchKernelGGL((scaled_fp8_quant_kernel<scalar_t, true>), grid, block, 0, s, o, in,
                         scale, hidden_size, in_row_stride, out_row_stride);
    } else {
      hipLaunchKernelGGL((absmax_to_scale_kernel<scalar_t, false>), grid, block, 0, s, scale,
                         in, hidden_size, in_row_stride);
      hipLaunchKernelGGL((scaled_fp8_quant_kernel<scalar_t, false>), grid, block, 0, s, o, in,
                         scale, hidden_size, in_row_stride, out_row_stride);
    }
    return check_launch("dynamic_scaled_fp8_quant");
  });
}

int mi355x_dynamic_per_token_scaled_fp8_quant(void* out, const void* input,
                                              float* scales, const float* scale_ub,
                                              int num_tokens, int hidden_size,
                                              int64_t in_row_stride,
                                              int64_t out_row_stride, int dtype,
                                              mi355x_stream stream) {
  MI355X_REQUIRE(num_tokens >= 0 && hidden_size > 0, MI355X_EINVAL,
                 "dynamic_per_token_scaled_fp8_quant: bad sizes");
  if (num_tokens == 0) return MI355X_OK;
  MI355X_REQUIRE(out && input && scales, MI355X_EINVAL,
                 "dynamic_per_token_scaled_fp8_quant: null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  return MI355X_DISPATCH_FLOAT(dtype, [&] {
    const scalar_t* in = static_cast<const scalar_t*>(input);
    uint8_t* o = static_cast<uint8_t*>(out);
    const bool vec = row_vec_ok<scalar_t>(in, o, hidden_size, in_row_stride, out_row_stride);
    dim3 grid(num_tokens), block(row_threads(hidden_size, vec ? 16 / sizeof(scalar_t) : 1));
    if (vec)
      hipLaunchKernelGGL((per_token_fp8_quant_kernel<scalar_t, true>), grid, block, 0, s, o,
                         scales, in, scale_ub, hidden_size, in_row_stride, out_row_stride);
    else
      hipLaunchKernelGGL((per_token_fp8_quant_kernel<scalar_t, false>), grid, block, 0, s, o,
                         scales, in, scale_ub, hidden_size, in_row_stride, out_row_stride);
    return check_launch("dynamic_per_token_scaled_fp8_quant");
  });
}

int mi355x_per_token_group_fp8_quant(void* out, float* scales, const void* input, int num_tokens,
                                     int hidden_size, int group_size, int64_t in_row_stride,
                                     int64_t out_row_stride, int64_t scale_row_stride,
                                     int64_t scale_group_stride, float eps, int dtype, mi355x_stream stream) {
  MI355X_REQUIRE(num_tokens >= 0 && hidden_size > 0, MI355X_EINVAL, "per_token_group_fp8_quant: bad sizes");
  MI355X_REQUIRE(group_size == 128, MI355X_EUNSUPPORTED,
                 "per_token_group_fp8_quant: group_size = %d, only 128 is supported", group_size);
  MI355X_REQUIRE(hidden_size % 128 == 0, MI355X_EUNSUPPORTED,
                 "per_token_group_fp8_quant: hidden_size = %d must be a multiple of 128", hidden_size);
  MI355X_REQUIRE(dtype == MI355X_F16 || dtype == MI355X_BF16, MI355X_EUNSUPPORTED,
                 "per_token_group_fp8_quant: input must be f16 or bf16");
  MI355X_REQUIRE(in_row_stride % 8 == 0 && out_row_stride % 8 == 0 && in_row_stride >= hidden_size &&
                     out_row_stride >= hidden_size && scale_row_stride >= 0 && scale_group_stride >= 0,
                 MI355X_EUNSUPPORTED, "per_token_group_fp8_quant: row strides must be multiples of 8 elements");
  if (num_tokens == 0) return MI355X_OK;
  MI355X_REQUIRE(out && scales && input, MI355X_EINVAL, "per_token_group_fp8_quant: null pointer");
  MI355X_REQUIRE((reinterpret_cast<uintptr_t>(input) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0,
                 MI355X_EUNSUPPORTED, "per_token_group_fp8_quant: input must be 16-byte, out 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  return MI355X_DISPATCH_HALF(dtype, [&] {
    hipLaunchKernelGGL((per_token_group_fp8_quant_kernel<scalar_t>), dim3(num_tokens),
                       dim3(row_threads(hidden_size, 8)), 0, s, static_cast<uint8_t*>(out), scales,
                       static_cast<const scalar_t*>(input), hidden_size, in_row_stride, out_row_stride,
                       scale_row_stride, scale_group_stride, eps);
    return check_launch("per_token_group_fp8_quant");
  });
}

int mi355x_per_token_group_fp8_quant_ue8m0(void* out, void* scales, int scale_elem_size, const void* input,
                                           int num_tokens, int hidden_size, int group_size, int64_t in_row_stride,
                                           int64_t out_row_stride, int64_t scale_row_stride,
                                           int64_t scale_group_stride, float eps, int dtype, mi355x_stream stream) {
  MI355X_REQUIRE(num_tokens >= 0 && hidden_size > 0, MI355X_EINVAL, "per_token_group_fp8_quant(ue8m0): bad sizes");
  MI355X_REQUIRE(group_size == 128 || group_size == 32, MI355X_EUNSUPPORTED,
                 "per_token_group_fp8_quant(ue8m0): group_size = %d, only 128 and 32 are supported", group_size);
  MI355X_REQUIRE(scale_elem_size == 1 || scale_elem_size == 4, MI355X_EUNSUPPORTED,
                 "per_token_group_fp8_quant(ue8m0): scales must be bytes or float32");
  MI355X_REQUIRE(hidden_size % group_size == 0, MI355X_EUNSUPPORTED,
                 "per_token_group_fp8_quant(ue8m0): hidden_size = %d must be a multiple of %d", hidden_size,
                 group_size);
  MI355X_REQUIRE(dtype == MI355X_F16 || dtype == MI355X_BF16, MI355X_EUNSUPPORTED,
                 "per_token_group_fp8_quant(ue8m0): input must be f16 or bf16");
  MI355X_REQUIRE(in_row_stride % 8 == 0 && out_row_stride % 8 == 0 && in_row_stride >= hidden_size &&
                     out_row_stride >= hidden_size && scale_row_stride >= 0 && scale_group_stride >= 0,
                 MI355X_EUNSUPPORTED, "per_token_group_fp8_quant(ue8m0): row strides must be multiples of 8 elements");
  if (num_tokens == 0) return MI355X_OK;
  MI355X_REQUIRE(out && scales && input, MI355X_EINVAL, "per_token_group_fp8_quant(ue8m0): null pointer");
  MI355X_REQUIRE((reinterpret_cast<uintptr_t>(input) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0,
                 MI355X_EUNSUPPORTED, "per_token_group_fp8_quant(ue8m0): input must be 16-byte, out 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  return MI355X_DISPATCH_HALF(dtype, [&] {
    auto launch = [&](auto kern, auto* sc) {
      hipLaunchKernelGGL(kern, dim3(num_tokens), dim3(row_threads(hidden_size, 8)), 0, s, static_cast<uint8_t*>(out),
                         sc, static_cast<const scalar_t*>(input), hidden_size, in_row_stride, out_row_stride,
                         scale_row_stride, scale_group_stride, eps);
    };
    uint8_t* sb = static_cast<uint8_t*>(scales);
    float* sf = static_cast<float*>(scales);
    if (scale_elem_size == 1) {
      if (group_size == 128) launch(per_token_group_fp8_quant_ue8m0_kernel<scalar_t, uint8_t, 16>, sb);
      else launch(per_token_group_fp8_quant_ue8m0_kernel<scalar_t, uint8_t, 4>, sb);
    } else {
      if (group_size == 128) launch(per_token_group_fp8_quant_ue8m0_kernel<scalar_t, float, 16>, sf);
      else launch(per_token_group_fp8_quant_ue8m0_kernel<scalar_t, float, 4>, sf);
    }
    return check_launch("per_token_group_fp8_quant(ue8m0)");
  });
}

}  // extern "C"
