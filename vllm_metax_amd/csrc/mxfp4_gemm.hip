// mxfp4_gemm.hip — MX-FP4 (OCP microscaling, w4a4) GEMM on the gfx950 scaled MFMA, and its activation quantiser.
// Elements are e2m1 nibbles (sign in bit 3, codes 0..7 = 0, 0.5, 1, 1.5, 2, 3, 4, 6; byte j of a row = element 2 j in
// the low nibble, 2 j + 1 in the high one: torch.float4_e2m1fn_x2), one E8M0 scale byte (2^(s - 127),
// torch.float8_e8m0fnu) per 32-wide K group on BOTH operands:
//     out[i, j] = T( sum_g 2^(a_s[i, g] - 127) 2^(b_s[g, j] - 127) (sum_{kk in group g} a[i, kk] b[kk, j]) + bias[j] )
// a [M, K / 2] bytes row-major, b [K / 2, N] column-major (a checkpoint's [N, K / 2] as its .t()), a_s [M, K / 32] and
// b_s [K / 32, N] with the group index contiguous; K % 128 == 0, N % 16 == 0.  The reference project has no MX path.
//
// MI355X design.  v_mfma_scale_f32_16x16x128_f8f6f4 in its fp4 form (cbsz = blgp = 4) takes 32 nibbles = 4 VGPRs per
// lane and operand and multiplies each lane's 32 products by 2^(scale - 127) of BOTH operands, the scale being one
// byte (op_sel) of a VGPR of that lane: a lane's nibbles are exactly one MX group.  So the scales never touch the
// vector ALU — every MFMA accumulates straight into the master accumulator (compare fp8_block_gemm.hip, whose fp32
// scales force zero-accumulator temporaries and a fold).  Which group a lane takes is free as long as A and B agree,
// and the order of the nibbles inside a group is free as well (both operands keep the memory order).
//   m <= 65  : mx4_stream_kernel — the stream structure of f8b_decode_kernel.  K runs in super-steps of 512 (4 MFMAs):
//              lane (lc = lane & 15, lr = lane >> 4) takes groups 4 lr + s in MFMA s, i.e. 64 contiguous bytes of
//              column lc (four dwordx4) and ONE aligned dword of scale bytes, picked with op_sel = s.  Weights and
//              their scale dwords go HBM -> VGPR through a register ring of super-steps; the activation nibbles and
//              scale dwords of the workgroup's K range are staged once in LDS in exactly the order the lanes read
//              them; no barrier in the loop; passes of 64 rows above 64.  A row costs 1/2 + 1/32 byte per k: the LDS
//              image is half the fp8 one, a workgroup's K range twice as long.  A ragged last super-step (K % 512 != 0:
//              r = 1..3 k-steps) runs the same code: lanes with lr >= r see a zeroed activation image and re-read
//              in-range weight bytes.
//   m  > 65  : mx4_tile_kernel — 256 x 256 tile on 8 waves, both operands read in place by whole-line LDS-DMA copies
//              (a 128-byte line is 256 k of one row; the staging of f8b_tile_kernel byte for byte), the stage's scale
//              dwords beside it by 4-byte LDS-DMA copies: 64 KiB + 4 KiB per stage, two stages.  Inside a stage lane lr
//              takes group lr of each of the two k-steps (16 bytes, scale byte read straight from LDS), so a K range
//              with an odd number of k-steps just skips the second half of its last stage.
// K split (both kernels) through fp32 slabs [sk][m][n] and mx4_finish_kernel, which adds them in slab order, adds the
// bias and rounds once: no memset, no atomics — deterministic and HIP-graph-replayable.
#include <cstdlib>

#include "w4a16.cuh"   // plan_tile_split

namespace mi355x {

typedef __attribute__((ext_vector_type(8))) int mx4_i32x8_t;

thread_local int mx4_route_mask = 0;

// acc += 2^(sa.byte[OP] - 127) 2^(sb.byte[OP] - 127) (16 x 16 x 128 e2m1 product); only the first 4 dwords of an fp4
// operand are read
template <int OP>
__device__ __forceinline__ f32x4_t mx4_mfma(uint4 a, uint4 b, f32x4_t c, uint32_t sa, uint32_t sb) {
  const mx4_i32x8_t av = {(int)a.x, (int)a.y, (int)a.z, (int)a.w, 0, 0, 0, 0};
  const mx4_i32x8_t bv = {(int)b.x, (int)b.y, (int)b.z, (int)b.w, 0, 0, 0, 0};
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, c, 4, 4, OP, (int)sa, OP, (int)sb);
}

// 64 x 4 bytes global -> LDS: lane l's dword lands at lds_base + 4 l (see lds_dma16, common.cuh)
__device__ __forceinline__ void mx4_lds_dma4(const void* gptr, uint32_t lds_base) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off" : : "v"(gptr), "s"(lds_base) : "memory");
}

struct Mx4Args {
  void* out;
  const uint8_t* a;
  const uint8_t* b;
  const uint8_t* a_scales;
  int64_t as_row;
  const uint8_t* b_scales;
  int64_t bs_col;
  const void* bias;
  float* ws;
  int64_t ws_elems;
  int m, n, k;
  int64_t lda, ldb, ldc;   // lda / ldb in bytes
  hipStream_t stream;
};

// ------------------------------------------------------------------------- stream kernel (passes of <= 64 rows)
// LDS: [super-steps][MT][4 lr][4 s][16 lc] uint4 activation image | [super-steps][MT][4 lr][16 lc] scale dwords
constexpr int kMx4ImgBytes = 4096, kMx4ScBytes = 256;   // per super-step and row tile

template <typename T, int MT, int NT>
__global__ __launch_bounds__(256) void mx4_stream_kernel(
    T* __restrict__ out, float* __restrict__ ws, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
    const uint8_t* __restrict__ a_scales, int64_t as_row, const uint8_t* __restrict__ b_scales, int64_t bs_col,
    const T* __restrict__ bias, int m, int n, int k, int64_t lda, int64_t ldb, int64_t ldc, int ss_per_split) {
  constexpr int D = 8 / NT;      // ring of weight super-steps, D - 1 in flight
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint4* a_img = reinterpret_cast<const uint4*>(smem);
  uint32_t* as_lds = reinterpret_cast<uint32_t*>(smem + (size_t)ss_per_split * MT * kMx4ImgBytes);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lc = lane & 15, lr = lane >> 4;
  const int total_steps = k >> 7;
  const int total_ss = (total_steps + 3) >> 2;
  const int ss0 = blockIdx.y * ss_per_split;
  const int nss = min(ss_per_split, total_ss - ss0);
  // k-steps of this range's last super-step (4 unless it is the ragged end of K): there lanes with lr >= r have no
  // groups; they re-read the bytes of lr = 0 (in range) against a zeroed activation image
  const int r = min(4, total_steps - (ss0 + nss - 1) * 4);
  const int fix = lr >= r ? 64 * lr : 0;
  const int n0 = (blockIdx.x * 4 + wave) * (16 * NT);
  const uint8_t* b_src[NT];
  const uint8_t* bs_src[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    int col = n0 + NT * lc + t;
    col = col < n ? col : n - 1;
    b_src[t] = b + (int64_t)col * ldb + (int64_t)ss0 * 256 + 64 * lr;
    bs_src[t] = b_scales + (int64_t)col * bs_col + ss0 * 16 + 4 * lr;
  }
  uint4 bq[D][NT][4];
  uint32_t bsc[D][NT];
  auto load_b = [&](int kk, uint4 (&dst)[NT][4], uint32_t (&dsc)[NT]) {
    const int kc = kk < nss ? kk : nss - 1;   // (clamped, not branched: beyond the range the last step is re-read)
    const int back = kc == nss - 1 ? fix : 0;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const uint8_t* p = b_src[t] + (kc * 256 - back);
#pragma unroll
      for (int s = 0; s < 4; ++s) dst[t][s] = *reinterpret_cast<const uint4*>(p + 16 * s);
      dsc[t] = *reinterpret_cast<const uint32_t*>(bs_src[t] + (kc * 16 - (back >> 4)));
    }
  };
#pragma unroll
  for (int s = 0; s < D - 1; ++s) load_b(s, bq[s], bsc[s]);
  {
    // activation image: one copy = (super-step, row tile, lr): lane (s = lane >> 4, row = lane & 15) brings 16 bytes,
    // 64 contiguous bytes per row; the copies are dealt round-robin to the waves
    const uint32_t lds_base = __builtin_amdgcn_readfirstlane(lds_addr_of(smem));
    const int copies = nss * MT * 4;
    for (int q = wave; q < copies; q += 4) {
      const int lrq = q & 3, i = (q >> 2) % MT, kk = (q >> 2) / MT;
      if (kk == nss - 1 && lrq >= r) {
        reinterpret_cast<uint4*>(smem)[q * 64 + lane] = make_uint4(0, 0, 0, 0);
        continue;
      }
      int row = 16 * i + lc;
      row = row < m ? row : m - 1;           // rows >= m only feed accumulator rows that are never stored
      lds_dma16(a + (int64_t)row * lda + (int64_t)(ss0 + kk) * 256 + 64 * lrq + 16 * lr, lds_base + q * 1024);
    }
    for (int idx = threadIdx.x; idx < nss * MT * 64; idx += 256) {
      const int kk = idx / (MT * 64);
      const int rest = idx - kk * (MT * 64);
      const int lrq = (rest >> 4) & 3;
      int row = 16 * (rest >> 6) + (rest & 15);
      row = row < m ? row : m - 1;
      uint32_t v = 0x7f7f7f7fu;
      if (!(kk == nss - 1 && lrq >= r))
        v = *reinterpret_cast<const uint32_t*>(a_scales + (int64_t)row * as_row + (ss0 + kk) * 16 + 4 * lrq);
      as_lds[idx] = v;
    }
    lds_dma_wait<0>();
  }
  __syncthreads();

  f32x4_t acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[i][t] = f32x4_t{0, 0, 0, 0};
  }
  auto mma = [&](int kk, uint4 (&cur)[NT][4], uint32_t (&csc)[NT]) {
    const uint4* ap = a_img + (kk * MT) * 256 + lr * 64 + lc;
    uint32_t asc[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) asc[i] = as_lds[(kk * MT + i) * 64 + lane];
#define MX4_STEP(S)                                                                              \
  _Pragma("unroll") for (int i = 0; i < MT; ++i) {                                               \
    const uint4 af = ap[i * 256 + (S) * 16];                                                     \
    _Pragma("unroll") for (int t = 0; t < NT; ++t)                                               \
        acc[i][t] = mx4_mfma<S>(af, cur[t][S], acc[i][t], asc[i], csc[t]);                       \
  }
    MX4_STEP(0)
    MX4_STEP(1)
    MX4_STEP(2)
    MX4_STEP(3)
#undef MX4_STEP
  };
  int kk = 0;
  for (; kk + D <= nss; kk += D) {
#pragma unroll
    for (int s = 0; s < D; ++s) {
      load_b(kk + s + D - 1, bq[(s + D - 1) % D], bsc[(s + D - 1) % D]);
      __builtin_amdgcn_sched_barrier(0);
      mma(kk + s, bq[s], bsc[s]);
    }
  }
#pragma unroll
  for (int s = 0; s < D - 1; ++s) {
    if (kk + s < nss) mma(kk + s, bq[s], bsc[s]);
  }

  // epilogue: NT adjacent columns per lane and row; a K split leaves its partial sums in slab blockIdx.y
  const int col0 = n0 + NT * lc;
  if (col0 >= n) return;
  const bool split = gridDim.y > 1;
  float bi[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) bi[t] = (bias && col0 + t < n) ? to_f32(bias[col0 + t]) : 0.f;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = i * 16 + 4 * lr + j;
      if (row >= m) continue;
      if (split) {
        float* dst = ws + ((int64_t)blockIdx.y * m + row) * n + col0;
#pragma unroll
        for (int t = 0; t < NT; ++t)
          if (col0 + t < n) dst[t] = acc[i][t][j];
      } else {
        T* dst = out + (int64_t)row * ldc + col0;
#pragma unroll
        for (int t = 0; t < NT; ++t)
          if (col0 + t < n) dst[t] = from_f32<T>(acc[i][t][j] + bi[t]);
      }
    }
  }
}

// ------------------------------------------------------------------------- tile kernel (m > 65)
constexpr int kMx4Piece = 2 * 16 * 64;          // uint4 per row half: 16 A + 16 B half tiles of 8 rows x 128 bytes
constexpr int kMx4Stage = 2 * kMx4Piece;        // 64 KiB: 256 rows + 256 columns of 256 k
constexpr int kMx4ScaleWords = 2 * 2 * 256;     // per stage: [A | B][k-step][row or column] dwords of 4 group bytes
constexpr size_t kMx4TileLds = (size_t)2 * kMx4Stage * 16 + 2 * kMx4ScaleWords * 4;

template <typename T>
__global__ __launch_bounds__(512, 2) void mx4_tile_kernel(
    T* __restrict__ out, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
    const uint8_t* __restrict__ a_scales, int64_t as_row, const uint8_t* __restrict__ b_scales, int64_t bs_col,
    const T* __restrict__ bias, int m, int n, int k, int64_t lda, int64_t ldb, int64_t ldc, int num_m_blocks,
    int num_tiles, float* __restrict__ slabs, int sk) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint4* lds = reinterpret_cast<const uint4*>(smem);
  const uint8_t* sc_lds = reinterpret_cast<const uint8_t*>(smem + (size_t)2 * kMx4Stage * 16);
  constexpr int kBOff = 16 * 64;
  // work item (tile, split), split-major; tiles dealt to the XCDs in contiguous runs, 8 row blocks per column block
  // (the order of f8b_tile_kernel)
  const int split = blockIdx.x / num_tiles;
  int mb, nb;
  {
    const int bid = blockIdx.x - split * num_tiles;
    const int q = num_tiles / 8, rr = num_tiles % 8;
    const int xcd = bid % 8;
    const int tile = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + bid / 8;
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
  // this split's K range in k-steps of 128; a stage is two of them, the last stage may hold one
  const int steps_all = k >> 7;
  const int per_split = (steps_all + sk - 1) / sk;
  const int ks0 = split * per_split;
  const int ksteps = max(0, min(per_split, steps_all - ks0));
  const int kstages = (ksteps + 1) >> 1;

  // operands in place: lane -> (row of a half tile, 16-byte chunk of the stage's 128-byte line), slot rotation as in
  // f8b_tile_kernel; weight piece 4 G + t holds columns 64 G + 4 r + t, so a lane ends up with 4 adjacent outputs.
  // Chunks 0-3 are the stage's first k-step, 4-7 its second: in a half stage those lanes re-read chunks 0-3.
  const uint8_t* a_src[2][2];
  const uint8_t* b_src[2][2];
  const int rm_row = lane >> 3, rm_chunk = (lane & 7) ^ ((lane >> 3) & 6);
  const int half_back = (rm_chunk & 4) ? 64 : 0;
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
  // scale copies: wave w brings the dwords of k-step w >> 2 of the stage for rows AND columns 64 (w & 3) + lane
  const uint8_t* sa_src;
  const uint8_t* sb_src;
  {
    int row = mb * 256 + (wave & 3) * 64 + lane;
    row = row < m ? row : m - 1;
    int col = nb * 256 + (wave & 3) * 64 + lane;
    col = col < n ? col : n - 1;
    sa_src = a_scales + (int64_t)row * as_row + 4 * (wave >> 2);
    sb_src = b_scales + (int64_t)col * bs_col + 4 * (wave >> 2);
  }
  const uint32_t lds_base = __builtin_amdgcn_readfirstlane(lds_addr_of(smem));
  const uint32_t sc_base = lds_base + 2 * kMx4Stage * 16;
  auto stage = [&](int buf, int st) {
    const bool half = 2 * st + 1 >= ksteps;
    const int64_t koff = (int64_t)(ks0 + 2 * st) * 64 - (half ? half_back : 0);
#pragma unroll
    for (int pp = 0; pp < 2; ++pp) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int dst = buf * kMx4Stage + pp * kMx4Piece + (wave * 2 + i) * 64;
        lds_dma16(a_src[i][pp] + koff, lds_base + dst * 16);
        lds_dma16(b_src[i][pp] + koff, lds_base + (dst + kBOff) * 16);
      }
    }
    if (!(half && wave >= 4)) {
      const int soff = (ks0 + 2 * st) * 4;
      mx4_lds_dma4(sa_src + soff, sc_base + (buf * kMx4ScaleWords + wave * 64) * 4);
      mx4_lds_dma4(sb_src + soff, sc_base + (buf * kMx4ScaleWords + 512 + wave * 64) * 4);
    }
  };

  f32x4_t acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[i][t] = f32x4_t{0, 0, 0, 0};
  }
  const int frag0 = (lc >> 3) * kMx4Piece + 8 * (lc & 7) + (lr ^ (lc & 6));   // chunk lr of row lc; ^ 4: chunk 4 + lr
  int cur = 0;
  if (kstages > 0) stage(0, 0);
  for (int st = 0; st < kstages; ++st) {
    lds_dma_wait<0>();
    __syncthreads();
    if (st + 1 < kstages) stage(cur ^ 1, st + 1);    // (slot cur ^ 1: its readers passed the barrier above)
    const uint4* abuf = lds + cur * kMx4Stage + (wm * 8) * 64;
    const uint4* bbuf = lds + cur * kMx4Stage + kBOff + (wn * 4) * 64;
    // scale byte lr of the dword of (k-step, row / column)
    const uint8_t* sa = sc_lds + (cur * kMx4ScaleWords + wm * 128 + lc) * 4 + lr;
    const uint8_t* sb = sc_lds + (cur * kMx4ScaleWords + 512 + wn * 64 + 4 * lc) * 4 + lr;
    const int nks = 2 * st + 1 >= ksteps ? 1 : 2;
    for (int s = 0; s < nks; ++s) {
      const int frag = frag0 ^ (4 * s);
      uint4 bf[4];
      uint32_t bs[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        bf[t] = bbuf[t * 64 + frag];
        bs[t] = sb[s * 1024 + t * 4];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const uint4 af = abuf[i * 64 + frag];
        const uint32_t as = sa[s * 1024 + i * 64];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[i][t] = mx4_mfma<0>(af, bf[t], acc[i][t], as, bs[t]);
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
__global__ __launch_bounds__(256) void mx4_finish_kernel(T* __restrict__ out, const float* __restrict__ ws,
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
static int mx4_launch_finish(const Mx4Args& g, int sk) {
  mx4_route_mask |= MI355X_MX4_ROUTE_SUM_SLABS;
  const int64_t threads = (int64_t)g.m * (g.n / 4);
  hipLaunchKernelGGL((mx4_finish_kernel<T>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, g.stream,
                     static_cast<T*>(g.out), g.ws, static_cast<const T*>(g.bias), g.m, g.n, g.ldc, sk);
  return check_launch("scaled_mm_mxfp4(finish)");
}

// plan of the stream kernel: the cost model of plan_block_decode (fp8_block_gemm.hip) in super-steps of 512 k — a
// workgroup of 64 NT columns streams 64 NT x 272 bytes per super-step (256 of nibbles, 16 of scales); NT column tiles
// per wave (2 at most: the ring holds 8 / NT super-steps of 17 VGPRs per column), sk K splits of `ss` super-steps,
// the activation image of a split <= 128 KiB.
struct Mx4StreamPlan {
  int nt, sk, ss;
};
static bool plan_mx4_stream(int m, int n, int k, int64_t ws_elems, Mx4StreamPlan* p) {
  const int total = (k + 511) / 512;
  const int mt = m <= 16 ? 1 : (m <= 32 ? 2 : 4);
  const int max_ss = (128 * 1024) / (mt * kMx4ImgBytes);
  double best = 1e30;
  bool found = false;
  for (int nt = 2; nt >= 1; nt >>= 1) {
    const int nblk = (n + 64 * nt - 1) / (64 * nt);
    for (int sk = 1; sk <= 16 && sk <= total; ++sk) {
      const int ss = (total + sk - 1) / sk;
      if ((total + ss - 1) / ss != sk || ss > max_ss) continue;
      if (sk > 1 && (int64_t)sk * m * n > ws_elems) continue;
      const int wgs = nblk * sk;
      const int img = mt * ss * (kMx4ImgBytes + kMx4ScBytes);
      int per_cu = (160 * 1024) / img;
      per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);
      const int rounds = (wgs + 256 * per_cu - 1) / (256 * per_cu);
      const int active = wgs < 256 ? wgs : 256;
      double rate = 6000.0 / active;              // GB/s per CU
      if (rate > 45.0) rate = 45.0;
      int conc = (wgs + 255) / 256;
      if (conc > per_cu) conc = per_cu;
      const double step_us = 17.4 * nt / rate * conc;
      double t = 5.5 + rounds * (img / 1024.0 / 68.0 + ss * step_us);
      if (sk > 1) t += 3.5 + 2.0 * (double)sk * m * n * 4 / 4e6;
      if (t < best) {
        best = t;
        *p = Mx4StreamPlan{nt, sk, ss};
        found = true;
      }
    }
  }
  return found;
}

template <typename T, int MT, int NT>
static int launch_mx4_stream(const Mx4Args& g, const Mx4StreamPlan& p) {
  auto kern = mx4_stream_kernel<T, MT, NT>;
  constexpr int kMaxLds = 144 * 1024;   // 128 KiB of image + its scales
  const size_t smem = (size_t)p.ss * MT * (kMx4ImgBytes + kMx4ScBytes);
  static PerDeviceOnce once;   // one per instantiation
  int dev;
  if (once.need(&dev)) {
    const hipError_t e =
        hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
    if (e != hipSuccess) {
      set_error("scaled_mm_mxfp4(stream): cannot reserve %d B of LDS: %s", kMaxLds, hipGetErrorString(e));
      return MI355X_EUNSUPPORTED;
    }
    once.mark(dev);
  }
  mx4_route_mask |= MI355X_MX4_ROUTE_STREAM;
  const int nblk = (g.n + 64 * NT - 1) / (64 * NT);
  hipLaunchKernelGGL(kern, dim3(nblk, p.sk), dim3(256), smem, g.stream, static_cast<T*>(g.out), g.ws, g.a, g.b,
                     g.a_scales, g.as_row, g.b_scales, g.bs_col, static_cast<const T*>(g.bias), g.m, g.n, g.k, g.lda,
                     g.ldb, g.ldc, p.ss);
  const int rc = check_launch("scaled_mm_mxfp4(stream)");
  if (rc || p.sk == 1) return rc;
  return mx4_launch_finish<T>(g, p.sk);
}

// one pass of <= 64 rows
template <typename T>
static int run_mx4_stream(const Mx4Args& g, const Mx4StreamPlan& p) {
#define MX4_NT(MTV) (p.nt == 2 ? launch_mx4_stream<T, MTV, 2>(g, p) : launch_mx4_stream<T, MTV, 1>(g, p))
  if (g.m <= 16) return MX4_NT(1);
  if (g.m <= 32) return MX4_NT(2);
  return MX4_NT(4);
#undef MX4_NT
}

template <typename T>
static int run_mx4_tile(const Mx4Args& g) {
  int sk = 1;
  if (g.ws != nullptr) sk = plan_tile_split(g.m, g.n, g.k / 128, g.ws_elems, 0);
  static PerDeviceOnce once;
  int dev;
  if (once.need(&dev)) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(mx4_tile_kernel<T>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMx4TileLds);
    if (e != hipSuccess) {
      set_error("scaled_mm_mxfp4(tile): cannot reserve %zu B of LDS: %s", kMx4TileLds, hipGetErrorString(e));
      return MI355X_EUNSUPPORTED;
    }
    once.mark(dev);
  }
  mx4_route_mask |= MI355X_MX4_ROUTE_TILE;
  const int num_m_blocks = (g.m + 255) / 256, num_n_blocks = (g.n + 255) / 256;
  const int num_tiles = num_m_blocks * num_n_blocks;
  hipLaunchKernelGGL((mx4_tile_kernel<T>), dim3(num_tiles * sk), dim3(512), kMx4TileLds, g.stream,
                     static_cast<T*>(g.out), g.a, g.b, g.a_scales, g.as_row, g.b_scales, g.bs_col,
                     static_cast<const T*>(g.bias), g.m, g.n, g.k, g.lda, g.ldb, g.ldc, num_m_blocks, num_tiles, g.ws,
                     sk);
  const int rc = check_launch("scaled_mm_mxfp4(tile)");
  if (rc || sk == 1) return rc;
  return mx4_launch_finish<T>(g, sk);
}

// Router.  m <= 65: passes of 64 rows through the stream kernel, above: the tile kernel.  The other scaled paths
// switch at 320, but the fp4 tile kernel with its K split overtakes a SECOND stream pass at once: forced either way
// on the Llama-3-70B TP = 8 shapes the stream kernel wins only at m <= 64 (profiles/mxfp4_gemm.txt); m = 65 keeps the
// two-pass form (64 rows + 1) alive and tested.  MI355X_MX4_TILE_MIN_M for A/B runs.  A shape the stream kernel has
// no plan for (a K range too long for LDS and no workspace to split it) goes to the tile kernel whatever m is.
static int mx4_tile_min_m() {
  static const int v = [] { const char* e = getenv("MI355X_MX4_TILE_MIN_M"); return e ? atoi(e) : 66; }();
  return v;
}

template <typename T>
static int run_mx4(const Mx4Args& g) {
  if (g.m < mx4_tile_min_m()) {
    Mx4StreamPlan plans[2];   // full passes, the ragged last one
    const int tail = g.m % 64;
    bool ok = true;
    if (g.m >= 64) ok = plan_mx4_stream(64, g.n, g.k, g.ws_elems, &plans[0]);
    if (ok && tail) ok = plan_mx4_stream(tail, g.n, g.k, g.ws_elems, &plans[1]);
    if (ok) {
      for (int row0 = 0; row0 < g.m; row0 += 64) {
        Mx4Args p = g;
        p.m = g.m - row0 < 64 ? g.m - row0 : 64;
        p.a = g.a + (int64_t)row0 * g.lda;
        p.out = static_cast<T*>(g.out) + (int64_t)row0 * g.ldc;
        p.a_scales = g.a_scales + (int64_t)row0 * g.as_row;
        const int rc = run_mx4_stream<T>(p, plans[p.m == 64 ? 0 : 1]);
        if (rc) return rc;
      }
      return MI355X_OK;
    }
  }
  return run_mx4_tile<T>(g);
}

// ------------------------------------------------------------------------- activation quantiser
// Per token and 32-wide group: e = amax rounded to the nearest value e2m1 can top out at, as an exponent
// (((bits(amax) + 0x200000) >> 23) & 0xFF: mantissas >= 1.75 carry into the next one), s = clamp(e - 2, 0, 254),
// q = sat_rne_e2m1(x 2^(127 - s)) with ties to the even code.  One pass: a lane pair holds a group (16 elements = two
// 16-byte loads per lane), the group's amax is one cross-lane step, no LDS; each lane stores its 8 bytes of nibbles,
// the even lane the scale byte.  Plain compares rather than v_cvt_scalef32_pk_fp4_*: the tie rule is part of the
// contract and the comparison form states it.
__device__ __forceinline__ uint32_t mx4_e2m1(float y) {
  const float v = fabsf(y);
  const uint32_t code = (v > 0.25f) + (v >= 0.75f) + (v > 1.25f) + (v >= 1.75f) + (v > 2.5f) + (v >= 3.5f) + (v > 5.f);
  return code | ((__float_as_uint(y) >> 28) & 8u);
}

template <typename T>
__global__ __launch_bounds__(256) void mxfp4_quant_kernel(uint8_t* __restrict__ q, uint8_t* __restrict__ s,
                                                          const T* __restrict__ in, int64_t halves, int groups,
                                                          int64_t in_stride, int64_t q_stride, int64_t s_stride) {
  static_assert(sizeof(T) == 2, "8 elements per 16-byte load");
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;   // half group; pairs never straddle the end
  const bool live = idx < halves;
  const int64_t h = live ? idx : halves - 1;
  const int64_t token = h / (2 * groups);
  const int hg = (int)(h - token * (2 * groups));
  const T* src = in + token * in_stride + hg * 16;
  T v[16];
  *reinterpret_cast<uint4*>(v) = *reinterpret_cast<const uint4*>(src);
  *reinterpret_cast<uint4*>(v + 8) = *reinterpret_cast<const uint4*>(src + 8);
  float x[16];
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    x[j] = to_f32(v[j]);
    amax = fmaxf(amax, fabsf(x[j]));
  }
  amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
  const int e = (int)(((__float_as_uint(amax) + 0x200000u) >> 23) & 0xFFu);
  const int sb = min(max(e - 2, 0), 254);
  uint32_t w[2] = {0, 0};
#pragma unroll
  for (int j = 0; j < 16; ++j) w[j >> 3] |= mx4_e2m1(__builtin_ldexpf(x[j], 127 - sb)) << (4 * (j & 7));
  if (!live) return;
  *reinterpret_cast<uint2*>(q + token * q_stride + hg * 8) = make_uint2(w[0], w[1]);
  if ((hg & 1) == 0) s[token * s_stride + (hg >> 1)] = (uint8_t)sb;
}

}  // namespace mi355x

using namespace mi355x;

extern "C" int mi355x_scaled_mm_mxfp4_last_route(void) { return mx4_route_mask; }

extern "C" int64_t mi355x_scaled_mm_mxfp4_workspace_elems(int m, int n, int k) {
  if (m <= 0 || n <= 0 || k <= 0 || k % 128 != 0) return 0;
  if (m < mx4_tile_min_m()) return (int64_t)8 * (m < 64 ? m : 64) * n;
  const int sk = plan_tile_split(m, n, k / 128, INT64_MAX, 0);
  return sk > 1 ? (int64_t)sk * m * n : 0;
}

extern "C" int mi355x_scaled_mm_mxfp4(void* out, const void* a, const void* b, const void* a_scales,
                                      int64_t a_s_row_stride, const void* b_scales, int64_t b_s_col_stride,
                                      const void* bias, float* workspace, int64_t workspace_elems, int m, int n, int k,
                                      int64_t lda, int64_t ldb, int64_t ldc, int out_dtype, mi355x_stream stream) {
  mx4_route_mask = 0;
  MI355X_REQUIRE(m >= 0 && n > 0 && k > 0, MI355X_EINVAL, "scaled_mm_mxfp4: bad sizes");
  MI355X_REQUIRE(k % 128 == 0, MI355X_EUNSUPPORTED, "scaled_mm_mxfp4: k = %d must be a multiple of 128", k);
  MI355X_REQUIRE(n % 16 == 0, MI355X_EUNSUPPORTED, "scaled_mm_mxfp4: n = %d must be a multiple of 16", n);
  MI355X_REQUIRE(lda % 16 == 0 && ldb % 16 == 0 && lda >= k / 2 && ldb >= k / 2, MI355X_EUNSUPPORTED,
                 "scaled_mm_mxfp4: lda / ldb must be multiples of 16 bytes, >= k / 2");
  MI355X_REQUIRE(ldc % 8 == 0 && ldc >= n, MI355X_EUNSUPPORTED,
                 "scaled_mm_mxfp4: rows of out must be multiples of 16 bytes, >= n elements");
  MI355X_REQUIRE(a_s_row_stride % 4 == 0 && b_s_col_stride % 4 == 0 && a_s_row_stride >= k / 32 &&
                     b_s_col_stride >= k / 32,
                 MI355X_EUNSUPPORTED, "scaled_mm_mxfp4: scale rows must be multiples of 4 bytes, >= k / 32");
  MI355X_REQUIRE(workspace_elems >= 0, MI355X_EINVAL, "scaled_mm_mxfp4: negative workspace size");
  if (m == 0) return MI355X_OK;
  MI355X_REQUIRE(out && a && b && a_scales && b_scales, MI355X_EINVAL, "scaled_mm_mxfp4: null pointer");
  MI355X_REQUIRE(((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) |
                   reinterpret_cast<uintptr_t>(out)) & 15) == 0,
                 MI355X_EUNSUPPORTED, "scaled_mm_mxfp4: a, b and out must be 16-byte aligned");
  MI355X_REQUIRE(((reinterpret_cast<uintptr_t>(a_scales) | reinterpret_cast<uintptr_t>(b_scales)) & 3) == 0,
                 MI355X_EUNSUPPORTED, "scaled_mm_mxfp4: the scales must be 4-byte aligned");
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) workspace = nullptr;   // slabs are stored 16 bytes at a time
  Mx4Args g{out, static_cast<const uint8_t*>(a), static_cast<const uint8_t*>(b),
            static_cast<const uint8_t*>(a_scales), a_s_row_stride, static_cast<const uint8_t*>(b_scales),
            b_s_col_stride, bias, workspace, workspace ? workspace_elems : 0, m, n, k, lda, ldb, ldc,
            static_cast<hipStream_t>(stream)};
  return MI355X_DISPATCH_HALF(out_dtype, [&] { return run_mx4<scalar_t>(g); });
}

extern "C" int mi355x_per_token_group_mxfp4_quant(void* out_q, void* out_s, const void* input, int num_tokens,
                                                  int hidden_size, int64_t in_row_stride, int64_t q_row_stride,
                                                  int64_t s_row_stride, int dtype, mi355x_stream stream) {
  MI355X_REQUIRE(num_tokens >= 0 && hidden_size > 0, MI355X_EINVAL, "per_token_group_mxfp4_quant: bad sizes");
  MI355X_REQUIRE(hidden_size % 32 == 0, MI355X_EUNSUPPORTED,
                 "per_token_group_mxfp4_quant: hidden_size = %d must be a multiple of 32", hidden_size);
  MI355X_REQUIRE(dtype == MI355X_F16 || dtype == MI355X_BF16, MI355X_EUNSUPPORTED,
                 "per_token_group_mxfp4_quant: input must be f16 or bf16");
  MI355X_REQUIRE(in_row_stride % 8 == 0 && in_row_stride >= hidden_size && q_row_stride % 8 == 0 &&
                     q_row_stride >= hidden_size / 2 && s_row_stride >= hidden_size / 32,
                 MI355X_EUNSUPPORTED,
                 "per_token_group_mxfp4_quant: rows of the input must be multiples of 16 bytes, of q of 8 bytes");
  if (num_tokens == 0) return MI355X_OK;
  MI355X_REQUIRE(out_q && out_s && input, MI355X_EINVAL, "per_token_group_mxfp4_quant: null pointer");
  MI355X_REQUIRE((reinterpret_cast<uintptr_t>(input) & 15) == 0 && (reinterpret_cast<uintptr_t>(out_q) & 7) == 0,
                 MI355X_EUNSUPPORTED, "per_token_group_mxfp4_quant: input must be 16-byte, q 8-byte aligned");
  const int groups = hidden_size / 32;
  const int64_t halves = (int64_t)num_tokens * groups * 2;
  return MI355X_DISPATCH_HALF(dtype, [&] {
    hipLaunchKernelGGL((mxfp4_quant_kernel<scalar_t>), dim3((unsigned)((halves + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), static_cast<uint8_t*>(out_q), static_cast<uint8_t*>(out_s),
                       static_cast<const scalar_t*>(input), halves, groups, in_row_stride, q_row_stride, s_row_stride);
    return check_launch("per_token_group_mxfp4_quant");
  });
}
