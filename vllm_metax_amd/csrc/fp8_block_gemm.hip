// fp8_block_gemm.hip — block-scaled FP8 (OCP e4m3fn) GEMM on gfx950 MFMA: the weights carry one fp32 scale per
// 128 x 128 block (a checkpoint's `weight_scale_inv`, weight_block_size = [128, 128]), the activations one per token
// and 128-wide K group (per_token_group_fp8_quant, fp8_quant.hip).  The reference names the capability
// (cutlass_scaled_mm_supports_block_fp8, csrc/torch_bindings.cpp:273-278) and answers false; semantics after its
// test-side definition tests/kernels/quant_utils.py (native_w8a8_block_matmul), restated:
//     out[i, j] = T( sum_kb a_s[i, kb] * b_s[kb, j / 128] * (sum_{kk in block kb} a[i, kk] * b[kk, j]) + bias[j] )
// a [M, K] row-major, b [K, N] column-major, a_s [M, KB], b_s [KB, NB] (both with free strides), KB = K / 128,
// NB = ceil(N / 128); K % 128 == 0, N % 16 == 0.
//
// MI355X design.  v_mfma_scale_f32_16x16x128_f8f6f4 has a K extent of exactly one scale block, so a k-step never
// straddles two blocks — but its own block scales are E8M0 powers of two and cannot carry an fp32 scale.  Every
// 128-k partial product therefore starts from a ZERO accumulator and is folded into an fp32 master accumulator on the
// vector ALU:  acc += t * (a_s[row, kb] * b_s[kb, col block]),  the product of the two scales formed once per
// (row, k-step).  A wave's columns always lie inside one 128-column block (its range starts at a multiple of its
// width, which divides 128), so b_s is wave-uniform per k-step; a_s is staged in LDS next to the activations.
//   m <= 320 : f8b_decode_kernel — the stream structure of gemm8_decode_kernel (fp8_gemm.hip): weights HBM -> VGPR
//              through a register ring of k-steps, the activation rows AND the scales of the workgroup's K range staged
//              once in LDS, no barrier in the loop; passes of 64 rows above 64.  All MT x NT MFMAs of a k-step go into
//              temporaries of their own before the first fold, so no fma waits for the MFMA it follows.
//   m  > 320 : f8b_tile_kernel — 256 x 256 tile on 8 waves, both operands read in place by whole-line LDS-DMA copies,
//              two 64-KiB stages of one 128-k block each (the AROW / BROW form of gemm8_packed_kernel); the scales of a
//              stage (256 a_s + the tile's 2 b_s) travel into LDS by 4-byte LDS-DMA copies with the stage itself, so
//              the loop holds no load the compiler's wait-count pass could tie to the copies.  A stage's 32 MFMAs run
//              in 4 groups of 8 into temporaries; each group is folded (16 packed fmas + 8 scale products) while the
//              SIMD's other wave and the next group keep the MFMA pipe busy.
// K split (both kernels) through fp32 slabs [sk][m][n] that already hold SCALED partial sums; f8b_finish_kernel adds
// them in slab order, adds the bias and rounds once: no memset, no atomics — deterministic and HIP-graph-replayable.
#include <cstdlib>

#include "w4a16.cuh"   // plan_tile_split

namespace mi355x {

typedef __attribute__((ext_vector_type(8))) int f8b_i32x8_t;

thread_local int f8b_route_mask = 0;

// one 16 x 16 x 128 e4m3 product from a zero accumulator (cbsz = blgp = 0: e4m3 on both sides; E8M0 scales 127 = 2^0)
__device__ __forceinline__ f32x4_t f8b_mfma(uint4 a0, uint4 a1, uint4 b0, uint4 b1) {
  const f8b_i32x8_t a = {(int)a0.x, (int)a0.y, (int)a0.z, (int)a0.w, (int)a1.x, (int)a1.y, (int)a1.z, (int)a1.w};
  const f8b_i32x8_t b = {(int)b0.x, (int)b0.y, (int)b0.z, (int)b0.w, (int)b1.x, (int)b1.y, (int)b1.z, (int)b1.w};
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0, 127, 0, 127);
}

// 64 x 4 bytes global -> LDS: lane l's dword lands at lds_base + 4 l (see lds_dma16, common.cuh)
__device__ __forceinline__ void lds_dma4(const void* gptr, uint32_t lds_base) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off" : : "v"(gptr), "s"(lds_base) : "memory");
}

struct F8bArgs {
  void* out;
  const uint8_t* a;
  const uint8_t* b;
  const float* a_scales;
  int64_t as_row, as_kb;
  const float* b_scales;
  int64_t bs_kb, bs_nb;
  const void* bias;
  float* ws;
  int64_t ws_elems;
  int m, n, k;
  int64_t lda, ldb, ldc;
  hipStream_t stream;
};

// ------------------------------------------------------------------------- decode (passes of <= 64 rows)
// LDS: [steps][MT][2][64] uint4 activation image (as gemm8_decode_kernel) | [steps][16 MT] a_s | [4 waves][steps] b_s
constexpr int kF8bStepBytes = 2048 + 64;   // per k-step and row tile: image + a_s (the 16 bytes of b_s come on top)

template <typename T, int MT, int NT>
__global__ __launch_bounds__(256) void f8b_decode_kernel(
    T* __restrict__ out, float* __restrict__ ws, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
    const float* __restrict__ a_scales, int64_t as_row, int64_t as_kb, const float* __restrict__ b_scales,
    int64_t bs_kb, int64_t bs_nb, const T* __restrict__ bias, int m, int n, int k, int64_t lda, int64_t ldb,
    int64_t ldc, int steps_per_split) {
  constexpr int D = 12 / NT;     // ring of weight k-steps, D - 1 in flight (gemm8_decode_kernel)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint4* a_img = reinterpret_cast<const uint4*>(smem);
  float* as_lds = reinterpret_cast<float*>(smem + (size_t)steps_per_split * MT * 2048);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* bs_lds = as_lds + steps_per_split * MT * 16 + wave * steps_per_split;
  const int lc = lane & 15, lr = lane >> 4;
  const int total_steps = k >> 7;
  const int kt0 = blockIdx.y * steps_per_split;
  const int nk = min(steps_per_split, total_steps - kt0);
  const int n0 = (blockIdx.x * 4 + wave) * (16 * NT);
  const uint8_t* b_src[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    int col = n0 + NT * lc + t;
    col = col < n ? col : n - 1;
    b_src[t] = b + (int64_t)col * ldb + (int64_t)kt0 * 128 + 16 * lr;
  }
  uint4 bq[D][NT][2];
  auto load_b = [&](int kk, uint4 (&dst)[NT][2]) {
    const int kc = kk < nk ? kk : nk - 1;     // (clamped, not branched: beyond the range the last step is re-read)
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      dst[t][0] = *reinterpret_cast<const uint4*>(b_src[t] + kc * 128);
      dst[t][1] = *reinterpret_cast<const uint4*>(b_src[t] + kc * 128 + 64);
    }
  };
#pragma unroll
  for (int s = 0; s < D - 1; ++s) load_b(s, bq[s]);
  {
    // activation image: whole-line copies, 8 rows x 128 bytes each, dealt round-robin to the waves
    const uint32_t lds_base = __builtin_amdgcn_readfirstlane(lds_addr_of(smem));
    const int copies = nk * 2 * MT;
    const int rm_row = lane >> 3, rm_chunk = (lane & 7) ^ ((lane >> 3) & 6);
    for (int q = wave; q < copies; q += 4) {
      const int j = q & 1, i = (q >> 1) % MT, kk = (q >> 1) / MT;
      int row = 16 * i + 8 * j + rm_row;
      row = row < m ? row : m - 1;           // rows >= m only feed accumulator rows that are never stored
      lds_dma16(a + (int64_t)row * lda + (int64_t)(kt0 + kk) * 128 + 16 * rm_chunk, lds_base + q * 1024);
    }
    // the scales of the K range: a_s [k-step][row], this wave's b_s [k-step] (its column block)
    for (int idx = threadIdx.x; idx < nk * MT * 16; idx += 256) {
      const int kk = idx / (MT * 16);
      int row = idx - kk * (MT * 16);
      row = row < m ? row : m - 1;
      as_lds[idx] = a_scales[row * as_row + (kt0 + kk) * as_kb];
    }
    const int nblk = (n + 127) >> 7;
    const int cb = min(n0 >> 7, nblk - 1);
    for (int kk = lane; kk < nk; kk += 64) bs_lds[kk] = b_scales[(kt0 + kk) * bs_kb + cb * bs_nb];
    lds_dma_wait<0>();
  }
  __syncthreads();

  f32x4_t acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[i][t] = f32x4_t{0, 0, 0, 0};
  }
  const int a_frag = (lc >> 3) * 64 + 8 * (lc & 7) + (lr ^ (lc & 6));
  const f32x4_t* as4 = reinterpret_cast<const f32x4_t*>(as_lds) + lr;   // rows 4 lr .. 4 lr + 3 of a row tile
  auto mma = [&](int kk, uint4 (&cur)[NT][2]) {
    const uint4* ap = a_img + (kk * MT) * 128;
    const float bsv = bs_lds[kk];
    f32x4_t tmp[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const uint4 a0 = ap[i * 128 + a_frag], a1 = ap[i * 128 + (a_frag ^ 4)];
#pragma unroll
      for (int t = 0; t < NT; ++t) tmp[i][t] = f8b_mfma(a0, a1, cur[t][0], cur[t][1]);
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const f32x4_t s = as4[(kk * MT + i) * 4] * bsv;
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[i][t] += tmp[i][t] * s;
    }
  };
  int kk = 0;
  for (; kk + D <= nk; kk += D) {
#pragma unroll
    for (int s = 0; s < D; ++s) {
      load_b(kk + s + D - 1, bq[(s + D - 1) % D]);
      __builtin_amdgcn_sched_barrier(0);
      mma(kk + s, bq[s]);
    }
  }
#pragma unroll
  for (int s = 0; s < D - 1; ++s) {
    if (kk + s < nk) mma(kk + s, bq[s]);
  }

  // epilogue: NT adjacent columns per lane and row; a K split leaves its scaled partial sums in slab blockIdx.y
  const int col0 = n0 + NT * lc;
  if (col0 >= n) return;
  const bool split = gridDim.y > 1;
  float bi[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) bi[t] = (bias && col0 + t < n) ? to_f32(bias[col0 + t]) : 0.f;
  const bool vec = (n % NT) == 0;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = i * 16 + 4 * lr + j;
      if (row >= m) continue;
      if (split) {
        float* dst = ws + ((int64_t)blockIdx.y * m + row) * n + col0;
        if (vec && NT == 4) {
          *reinterpret_cast<f32x4_t*>(dst) = f32x4_t{acc[i][0][j], acc[i][1][j], acc[i][2][j], acc[i][3][j]};
        } else {
#pragma unroll
          for (int t = 0; t < NT; ++t)
            if (col0 + t < n) dst[t] = acc[i][t][j];
        }
      } else {
        T o[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) o[t] = from_f32<T>(acc[i][t][j] + bi[t]);
        T* dst = out + (int64_t)row * ldc + col0;
        if (vec && NT == 4) {
          *reinterpret_cast<uint2*>(dst) = *reinterpret_cast<const uint2*>(o);
        } else {
#pragma unroll
          for (int t = 0; t < NT; ++t)
            if (col0 + t < n) dst[t] = o[t];
        }
      }
    }
  }
}

// ------------------------------------------------------------------------- tile kernel (m > 320)
constexpr int kF8bPiece = 2 * 16 * 64;          // uint4 per row half: 16 A + 16 B half tiles of 8 rows x 128 bytes
constexpr int kF8bStage = 2 * kF8bPiece;        // 64 KiB
constexpr int kF8bScaleFloats = 256 + 64;       // per stage: a_s of the tile's 256 rows, b_s of its 2 column blocks
constexpr size_t kF8bTileLds = (size_t)2 * kF8bStage * 16 + 2 * kF8bScaleFloats * 4;

template <typename T>
__global__ __launch_bounds__(512, 2) void f8b_tile_kernel(
    T* __restrict__ out, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
    const float* __restrict__ a_scales, int64_t as_row, int64_t as_kb, const float* __restrict__ b_scales,
    int64_t bs_kb, int64_t bs_nb, const T* __restrict__ bias, int m, int n, int k, int64_t lda, int64_t ldb,
    int64_t ldc, int num_m_blocks, int num_tiles, float* __restrict__ slabs, int sk) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint4* lds = reinterpret_cast<const uint4*>(smem);
  const float* sc_lds = reinterpret_cast<const float*>(smem + (size_t)2 * kF8bStage * 16);
  constexpr int kBOff = 16 * 64;
  // work item (tile, split), split-major; tiles dealt to the XCDs in contiguous runs, 8 row blocks per column block
  // (the order of gemm8_packed_kernel)
  const int split = blockIdx.x / num_tiles;
  int mb, nb;
  {
    const int bid = blockIdx.x - split * num_tiles;
    const int q = num_tiles / 8, r = num_tiles % 8;
    const int xcd = bid % 8;
    const int tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;
    constexpr int GM = 8;
    const int num_n_blocks = num_tiles / num_m_blocks;
    const int group = tile / (GM * num_n_blocks);
    const int first_m = group * GM;
    const int gsz = min(num_m_blocks - first_m, GM);
    const int within = tile - group * GM * num_n_blocks;
    mb = first_m + within % gsz;
    nb = within / gsz;
  }
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int lc = lane & 15, lr = lane >> 4;
  const int kstages_all = k >> 7;
  const int per_split = (kstages_all + sk - 1) / sk;
  const int ks0 = split * per_split;
  const int kstages = max(0, min(per_split, kstages_all - ks0));

  // operands in place: lane -> (row of a half tile, 16-byte chunk of the stage's 128 k bytes), slot rotation as in
  // gemm8_packed_kernel; weight piece 4 G + t holds columns 64 G + 4 r + t, so a lane ends up with 4 adjacent outputs
  const uint8_t* a_src[2][2];
  const uint8_t* b_src[2][2];
  const int rm_row = lane >> 3, rm_chunk = (lane & 7) ^ ((lane >> 3) & 6);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int p = wave * 2 + i;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      int row = mb * 256 + p * 16 + 8 * j + rm_row;
      row = row < m ? row : m - 1;            // rows >= m only feed accumulator rows that are never stored
      a_src[i][j] = a + (int64_t)row * lda + 16 * rm_chunk;
      int col = nb * 256 + 64 * (p >> 2) + 4 * (8 * j + rm_row) + (p & 3);
      col = col < n ? col : n - 1;
      b_src[i][j] = b + (int64_t)col * ldb + 16 * rm_chunk;
    }
  }
  // scale copies: waves 0-3 bring the a_s of 64 rows each, wave 4 the b_s of the tile's two column blocks
  const float* sc_src;
  {
    int row = mb * 256 + (wave & 3) * 64 + lane;
    row = row < m ? row : m - 1;
    const int nblk = (n + 127) >> 7;
    const int cb = min(nb * 2 + (lane & 1), nblk - 1);
    sc_src = wave < 4 ? a_scales + row * as_row : b_scales + cb * bs_nb;
  }
  const int64_t sc_step = wave < 4 ? as_kb : bs_kb;
  const uint32_t lds_base = __builtin_amdgcn_readfirstlane(lds_addr_of(smem));
  auto stage = [&](int buf, int ks) {
    const int64_t koff = (int64_t)(ks0 + ks) * 128;
#pragma unroll
    for (int pp = 0; pp < 2; ++pp) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int dst = buf * kF8bStage + pp * kF8bPiece + (wave * 2 + i) * 64;
        lds_dma16(a_src[i][pp] + koff, lds_base + dst * 16);
        lds_dma16(b_src[i][pp] + koff, lds_base + (dst + kBOff) * 16);
      }
    }
    if (wave < 5)
      lds_dma4(sc_src + (ks0 + ks) * sc_step, lds_base + 2 * kF8bStage * 16 + (buf * kF8bScaleFloats + wave * 64) * 4);
  };

  f32x4_t acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[i][t] = f32x4_t{0, 0, 0, 0};
  }
  const int rm2 = (lc >> 3) * kF8bPiece + 8 * (lc & 7) + (lr ^ (lc & 6));
  const int frag0 = rm2, frag1 = rm2 ^ 4;
  int cur = 0;
  if (kstages > 0) stage(0, 0);
  for (int ks = 0; ks < kstages; ++ks) {
    lds_dma_wait<0>();
    __syncthreads();
    if (ks + 1 < kstages) stage(cur ^ 1, ks + 1);    // (slot cur ^ 1: its readers passed the barrier above)
    const uint4* abuf = lds + cur * kF8bStage + (wm * 8) * 64;
    const uint4* bbuf = lds + cur * kF8bStage + kBOff + (wn * 4) * 64;
    const float* scb = sc_lds + cur * kF8bScaleFloats;
    const float bsv = scb[256 + (wn >> 1)];
    const f32x4_t* as4 = reinterpret_cast<const f32x4_t*>(scb + wm * 128) + lr;
    uint4 bf[4][2];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      bf[t][0] = bbuf[t * 64 + frag0];
      bf[t][1] = bbuf[t * 64 + frag1];
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      uint4 af[2][2];
      f32x4_t tmp[2][4];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        af[i][0] = abuf[(2 * g + i) * 64 + frag0];
        af[i][1] = abuf[(2 * g + i) * 64 + frag1];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int t = 0; t < 4; ++t) tmp[i][t] = f8b_mfma(af[i][0], af[i][1], bf[t][0], bf[t][1]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const f32x4_t s = as4[(2 * g + i) * 4] * bsv;    // a_s[row] * b_s once per (row, stage)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[2 * g + i][t] += tmp[i][t] * s;
      }
    }
    cur ^= 1;
  }

  const int col = nb * 256 + wn * 64 + 4 * lc;
  if (col >= n) return;
  float bi[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) bi[t] = bias ? to_f32(bias[col + t]) : 0.f;
  float* sl = slabs + (int64_t)split * m * n;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = mb * 256 + wm * 128 + i * 16 + 4 * lr + j;
      if (row >= m) continue;
      if (sk > 1) {
        *reinterpret_cast<f32x4_t*>(sl + (int64_t)row * n + col) =
            f32x4_t{acc[i][0][j], acc[i][1][j], acc[i][2][j], acc[i][3][j]};
      } else {
        T o[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) o[t] = from_f32<T>(acc[i][t][j] + bi[t]);
        *reinterpret_cast<uint2*>(out + (int64_t)row * ldc + col) = *reinterpret_cast<const uint2*>(o);
      }
    }
  }
}

// out = T(slab 0 + slab 1 + ... + bias), slabs added in index order; one thread = 4 adjacent columns of a row
template <typename T>
__global__ __launch_bounds__(256) void f8b_finish_kernel(T* __restrict__ out, const float* __restrict__ ws,
                                                         const T* __restrict__ bias, int m, int n, int64_t ldc,
                                                         int sk) {
  const int n4 = n >> 2;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)m * n4) return;
  const int row = (int)(idx / n4), col = (int)(idx - (int64_t)row * n4) * 4;
  float v[4];
  sum_slabs<4>(ws + (int64_t)row * n + col, sk, (int64_t)m * n, v);
  T o[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) o[t] = from_f32<T>(v[t] + (bias ? to_f32(bias[col + t]) : 0.f));
  *reinterpret_cast<uint2*>(out + (int64_t)row * ldc + col) = *reinterpret_cast<const uint2*>(o);
}

template <typename T>
static int launch_finish(const F8bArgs& g, const float* slabs, int sk) {
  f8b_route_mask |= MI355X_F8B_ROUTE_SUM_SLABS;
  const int64_t threads = (int64_t)g.m * (g.n / 4);
  hipLaunchKernelGGL((f8b_finish_kernel<T>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, g.stream,
                     static_cast<T*>(g.out), slabs, static_cast<const T*>(g.bias), g.m, g.n, g.ldc, sk);
  return check_launch("scaled_mm_fp8_block(finish)");
}

// plan of the decode kernel: the cost model of the row-scaled stream kernel (fp8_gemm.hip plan_decode, fitted to the
// same weight stream; the scale traffic is < 4 % of the activation image's): NT column tiles per wave, sk K splits
// of `steps` k-steps, the activation image of a split <= 128 KiB.
struct F8bDecodePlan {
  int nt, sk, steps;
};
static bool plan_block_decode(int m, int n, int k, int64_t ws_elems, F8bDecodePlan* p) {
  const int total = k / 128;
  const int mt = m <= 16 ? 1 : (m <= 32 ? 2 : 4);
  const int max_steps = (128 * 1024) / (mt * 2048);
  double best = 1e30;
  bool found = false;
  for (int nt = 4; nt >= 1; nt >>= 1) {
    const int nblk = (n + 64 * nt - 1) / (64 * nt);
    for (int sk = 1; sk <= 16 && sk <= total; ++sk) {
      const int steps = (total + sk - 1) / sk;
      if ((total + steps - 1) / steps != sk || steps > max_steps) continue;
      if (sk > 1 && (int64_t)sk * m * n > ws_elems) continue;
      const int wgs = nblk * sk;
      const int img = mt * steps * 2048;
      int per_cu = (160 * 1024) / img;
      per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);
      const int rounds = (wgs + 256 * per_cu - 1) / (256 * per_cu);
      const int active = wgs < 256 ? wgs : 256;
      double rate = 6000.0 / active;              // GB/s per CU
      if (rate > 45.0) rate = 45.0;
      int conc = (wgs + 255) / 256;
      if (conc > per_cu) conc = per_cu;
      const double step_us = 8.2 * nt / rate * conc;
      double t = 5.5 + rounds * (img / 1024.0 / 68.0 + steps * step_us);
      if (sk > 1) t += 3.5 + 2.0 * (double)sk * m * n * 4 / 4e6;
      if (t < best) {
        best = t;
        *p = F8bDecodePlan{nt, sk, steps};
        found = true;
      }
    }
  }
  return found;
}

template <typename T, int MT, int NT>
static int launch_block_decode(const F8bArgs& g, const F8bDecodePlan& p) {
  auto kern = f8b_decode_kernel<T, MT, NT>;
  constexpr int kMaxLds = 144 * 1024;   // 128 KiB of image + its scales
  const size_t smem = (size_t)p.steps * (MT * kF8bStepBytes + 16);
  static PerDeviceOnce once;   // one per instantiation
  int dev;
  if (once.need(&dev)) {
    const hipError_t e =
        hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
    if (e != hipSuccess) {
      set_error("scaled_mm_fp8_block(decode): cannot reserve %d B of LDS: %s", kMaxLds, hipGetErrorString(e));
      return MI355X_EUNSUPPORTED;
    }
    once.mark(dev);
  }
  f8b_route_mask |= MI355X_F8B_ROUTE_DECODE;
  const int nblk = (g.n + 64 * NT - 1) / (64 * NT);
  hipLaunchKernelGGL(kern, dim3(nblk, p.sk), dim3(256), smem, g.stream, static_cast<T*>(g.out), g.ws, g.a, g.b,
                     g.a_scales, g.as_row, g.as_kb, g.b_scales, g.bs_kb, g.bs_nb, static_cast<const T*>(g.bias), g.m,
                     g.n, g.k, g.lda, g.ldb, g.ldc, p.steps);
  const int rc = check_launch("scaled_mm_fp8_block(decode)");
  if (rc || p.sk == 1) return rc;
  return launch_finish<T>(g, g.ws, p.sk);
}

// one pass of <= 64 rows
template <typename T>
static int run_block_decode(const F8bArgs& g, const F8bDecodePlan& p) {
#define F8B_NT(MTV)                                             \
  (p.nt == 4 ? launch_block_decode<T, MTV, 4>(g, p)             \
             : (p.nt == 2 ? launch_block_decode<T, MTV, 2>(g, p) : launch_block_decode<T, MTV, 1>(g, p)))
  if (g.m <= 16) return F8B_NT(1);
  if (g.m <= 32) return F8B_NT(2);
  return F8B_NT(4);
#undef F8B_NT
}

template <typename T>
static int run_block_tile(const F8bArgs& g) {
  int sk = 1;
  if (g.ws != nullptr) sk = plan_tile_split(g.m, g.n, g.k / 128, g.ws_elems, 0);
  static PerDeviceOnce once;
  int dev;
  if (once.need(&dev)) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(f8b_tile_kernel<T>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)kF8bTileLds);
    if (e != hipSuccess) {
      set_error("scaled_mm_fp8_block(tile): cannot reserve %zu B of LDS: %s", kF8bTileLds, hipGetErrorString(e));
      return MI355X_EUNSUPPORTED;
    }
    once.mark(dev);
  }
  f8b_route_mask |= MI355X_F8B_ROUTE_TILE;
  const int num_m_blocks = (g.m + 255) / 256, num_n_blocks = (g.n + 255) / 256;
  const int num_tiles = num_m_blocks * num_n_blocks;
  hipLaunchKernelGGL((f8b_tile_kernel<T>), dim3(num_tiles * sk), dim3(512), kF8bTileLds, g.stream,
                     static_cast<T*>(g.out), g.a, g.b, g.a_scales, g.as_row, g.as_kb, g.b_scales, g.bs_kb, g.bs_nb,
                     static_cast<const T*>(g.bias), g.m, g.n, g.k, g.lda, g.ldb, g.ldc, num_m_blocks, num_tiles, g.ws,
                     sk);
  const int rc = check_launch("scaled_mm_fp8_block(tile)");
  if (rc || sk == 1) return rc;
  return launch_finish<T>(g, g.ws, sk);
}

// Router.  m <= 320: passes of 64 rows through the decode kernel (the weights of the second and later passes come
// from L2 / MALL), above: the tile kernel — the threshold of the row-scaled path (fp8_gemm.hip run_fp8), which moves
// the same bytes through the same two schedules; profiles/fp8_block_gemm.txt has both kernels on both sides of it.
// MI355X_F8B_TILE_MIN_M for A/B runs.  A shape the decode kernel has no plan for (a K range too long for LDS and
// no workspace to split it) goes to the tile kernel whatever m is.
template <typename T>
static int run_block(const F8bArgs& g) {
  static const int kTileMinM = [] { const char* e = getenv("MI355X_F8B_TILE_MIN_M"); return e ? atoi(e) : 321; }();
  if (g.m < kTileMinM) {
    const int64_t ws_elems = g.ws ? g.ws_elems : 0;
    F8bDecodePlan plans[2];   // full passes, the ragged last one
    const int tail = g.m % 64;
    bool ok = true;
    if (g.m >= 64) ok = plan_block_decode(64, g.n, g.k, ws_elems, &plans[0]);
    if (ok && tail) ok = plan_block_decode(tail, g.n, g.k, ws_elems, &plans[1]);
    if (ok) {
      for (int row0 = 0; row0 < g.m; row0 += 64) {
        F8bArgs p = g;
        p.m = g.m - row0 < 64 ? g.m - row0 : 64;
        p.a = g.a + (int64_t)row0 * g.lda;
        p.out = static_cast<T*>(g.out) + (int64_t)row0 * g.ldc;
        p.a_scales = g.a_scales + row0 * g.as_row;
        const int rc = run_block_decode<T>(p, plans[p.m == 64 ? 0 : 1]);
        if (rc) return rc;
      }
      return MI355X_OK;
    }
  }
  return run_block_tile<T>(g);
}

}  // namespace mi355x

using namespace mi355x;

extern "C" int mi355x_scaled_mm_block_last_route(void) { return f8b_route_mask; }

extern "C" int mi355x_scaled_mm_fp8_block(void* out, const void* a, const void* b, const float* a_scales,
                                          int64_t a_s_row_stride, int64_t a_s_kb_stride, const float* b_scales,
                                          int64_t b_s_kb_stride, int64_t b_s_nb_stride, const void* bias,
                                          float* workspace, int64_t workspace_elems, int m, int n, int k, int64_t lda,
                                          int64_t ldb, int64_t ldc, int out_dtype, mi355x_stream stream) {
  f8b_route_mask = 0;
  MI355X_REQUIRE(m >= 0 && n > 0 && k > 0, MI355X_EINVAL, "scaled_mm_fp8_block: bad sizes");
  MI355X_REQUIRE(k % 128 == 0, MI355X_EUNSUPPORTED, "scaled_mm_fp8_block: k = %d must be a multiple of 128", k);
  MI355X_REQUIRE(n % 16 == 0, MI355X_EUNSUPPORTED, "scaled_mm_fp8_block: n = %d must be a multiple of 16", n);
  MI355X_REQUIRE(lda % 16 == 0 && ldb % 16 == 0 && lda >= k && ldb >= k, MI355X_EUNSUPPORTED,
                 "scaled_mm_fp8_block: lda / ldb must be multiples of 16 bytes, >= k");
  MI355X_REQUIRE(ldc % 8 == 0 && ldc >= n, MI355X_EUNSUPPORTED,
                 "scaled_mm_fp8_block: rows of out must be multiples of 16 bytes, >= n elements");
  MI355X_REQUIRE(a_s_row_stride >= 0 && a_s_kb_stride >= 0 && b_s_kb_stride >= 0 && b_s_nb_stride >= 0,
                 MI355X_EINVAL, "scaled_mm_fp8_block: negative scale stride");
  MI355X_REQUIRE(workspace_elems >= 0, MI355X_EINVAL, "scaled_mm_fp8_block: negative workspace size");
  if (m == 0) return MI355X_OK;
  MI355X_REQUIRE(out && a && b && a_scales && b_scales, MI355X_EINVAL, "scaled_mm_fp8_block: null pointer");
  MI355X_REQUIRE(((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) |
                   reinterpret_cast<uintptr_t>(out)) & 15) == 0,
                 MI355X_EUNSUPPORTED, "scaled_mm_fp8_block: a, b and out must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) workspace = nullptr;   // slabs are stored 16 bytes at a time
  F8bArgs g{out, static_cast<const uint8_t*>(a), static_cast<const uint8_t*>(b), a_scales, a_s_row_stride,
            a_s_kb_stride, b_scales, b_s_kb_stride, b_s_nb_stride, bias, workspace, workspace ? workspace_elems : 0,
            m, n, k, lda, ldb, ldc, static_cast<hipStream_t>(stream)};
  return MI355X_DISPATCH_HALF(out_dtype, [&] { return run_block<scalar_t>(g); });
}
