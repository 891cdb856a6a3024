// fp8_e8m0_gemm.hip — FP8 (OCP e4m3fn) GEMM whose scales are E8M0 bytes (2^(s - 127), torch.float8_e8m0fnu) on BOTH
// operands, at two granularities:
//   block form (scale_group = 128): a_s [M, K / 128] per token and 128-wide K group, b_s [K / 128, ceil(N / 128)] per
//              128 x 128 weight block, any strides — block fp8 with `scale_fmt: ue8m0` (upstream's scale_ue8m0 = True);
//   MX form    (scale_group = 32) : a_s [M, K / 32], b_s [K / 32, N], the group index contiguous — OCP MXFP8.
//     out[i, j] = T( sum_g 2^(a_s[i, g] - 127) 2^(b_s[g, j or j / 128] - 127) (sum_{kk in group g} a[i, kk] b[kk, j])
//                    + bias[j] )
// a [M, K] row-major, b [K, N] column-major (a checkpoint's [N, K] as its .t()); K % 128 == 0, N % 16 == 0; fp32
// accumulation, ONE rounding.  Scale byte 255 (E8M0's NaN) is outside the contract: the MFMA's answer to it is not
// defined here.  The reference project has neither form.
//
// MI355X design.  v_mfma_scale_f32_16x16x128_f8f6f4 multiplies the 32 products of each 32-wide block of its K extent
// by 2^(scale - 127) of both operands; the scale of block g of row / column lc is one byte (op_sel) of a VGPR of lane
// 16 g + lc.  So the scales never touch the vector ALU: every MFMA accumulates straight into the master accumulator —
// no zero-started temporaries and no fold (compare fp8_block_gemm.hip, whose fp32 scales force both).  An fp8 operand
// is 8 VGPRs per lane, and lane group lr does NOT hold block lr: VGPRs 0-3 are bytes 16 lr .. 16 lr + 15 of the 128,
// VGPRs 4-7 bytes 64 + 16 lr .. — block g is the first halves of lane groups 0, 1 (g = 0), 2, 3 (g = 1) and their
// second halves (g = 2, 3).  (Measured: with one 32-byte group per lane the scale-placement test fails, with this
// layout it is bit-exact.)  Which memory group becomes which block is free as long as A, B and the scales agree.
// The granularity is a template switch (MX) that changes only where a lane fetches its scale byte; the loops are the
// same code.
//   m <= 65  : f8e_stream_kernel — passes of <= 64 rows.  K runs in super-steps of 512 (4 MFMAs over 4 lines of 128
//              bytes): block g of MFMA s is memory group 4 g + s, so lane group lr supplies the scales of line lr — MX
//              form: ONE aligned dword, picked with op_sel = s; block form: the line is ONE 128-k block, one byte — and
//              the data halves lr & 1 of the groups of lines lr >> 1 (VGPRs 0-3) and 2 + (lr >> 1) (VGPRs 4-7): eight
//              dwordx4 per column and super-step, a lane pair reading two whole lines.  Weights and their scales go
//              HBM -> VGPR through a register ring of super-steps; the activation rows of the workgroup's K range are
//              staged once in LDS by whole-line LDS-DMA copies (8 rows x 128 bytes, line = k-step), their scale bytes
//              beside them in read order; one barrier, none in the loop.  A ragged last super-step (K % 512 != 0:
//              r = 1..3 lines) runs the same code: lines >= r are zeroed in the activation image, and the lanes that
//              would read them re-read the in-range weight bytes and scales of line 0.
//   m  > 65  : f8e_tile_kernel — the in-place schedule of f8b_tile_kernel: 256 x 256 tile on 8 waves, two 64-KiB stages
//              of one 128-k step, both operands read where they lie by whole-line LDS-DMA copies; block g is group g
//              of the step (lane lr reads chunks lr and 4 + lr of the line, scale byte lr).  The stage's scale bytes
//              come beside it by 4-byte LDS-DMA copies — MX: the dword of (row | column, k-step), 2 KiB; block: the
//              ALIGNED dword that holds the byte (it cannot leave the byte's page), 256 + 2 of them — and are read
//              from LDS one byte per MFMA operand, so the loop holds no global load.
// K split (both kernels) through fp32 slabs [sk][m][n] and f8e_finish_kernel, which adds them in slab order, adds the
// bias and rounds once: no memset, no atomics — deterministic and HIP-graph-replayable.
#include <cstdlib>

#include "w4a16.cuh"   // plan_tile_split

namespace mi355x {

typedef __attribute__((ext_vector_type(8))) int f8e_i32x8_t;

thread_local int f8e_route_mask = 0;

// acc += 2^(sa.byte[OP] - 127) 2^(sb.byte[OP] - 127) (16 x 16 x 128 e4m3 product: cbsz = blgp = 0)
template <int OP>
__device__ __forceinline__ f32x4_t f8e_mfma(uint4 a0, uint4 a1, uint4 b0, uint4 b1, f32x4_t c, uint32_t sa,
                                            uint32_t sb) {
  const f8e_i32x8_t a = {(int)a0.x, (int)a0.y, (int)a0.z, (int)a0.w, (int)a1.x, (int)a1.y, (int)a1.z, (int)a1.w};
  const f8e_i32x8_t b = {(int)b0.x, (int)b0.y, (int)b0.z, (int)b0.w, (int)b1.x, (int)b1.y, (int)b1.z, (int)b1.w};
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, OP, (int)sa, OP, (int)sb);
}

// 64 x 4 bytes global -> LDS: lane l's dword lands at lds_base + 4 l (see lds_dma16, common.cuh)
__device__ __forceinline__ void f8e_lds_dma4(const void* gptr, uint32_t lds_base) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off" : : "v"(gptr), "s"(lds_base) : "memory");
}

struct F8eArgs {
  void* out;
  const uint8_t* a;
  const uint8_t* b;
  const uint8_t* a_scales;
  int64_t as_row, as_g;    // strides of a_s: row, K group
  const uint8_t* b_scales;
  int64_t bs_g, bs_c;      // strides of b_s: K group, column (MX) or column block
  const void* bias;
  float* ws;
  int64_t ws_elems;
  int m, n, k;
  int64_t lda, ldb, ldc;
  hipStream_t stream;
};

// ------------------------------------------------------------------------- stream kernel (passes of <= 64 rows)
// LDS: [k-steps][MT][2][64] uint4 activation image (8 rows x 128 bytes per copy) | [super-steps][MT][64] scale dwords
constexpr int kF8eImgBytes = 8192, kF8eScBytes = 256;   // per super-step and row tile

template <typename T, int MT, int NT, bool MX>
__global__ __launch_bounds__(256) void f8e_stream_kernel(
    T* __restrict__ out, float* __restrict__ ws, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
    const uint8_t* __restrict__ a_scales, int64_t as_row, int64_t as_g, const uint8_t* __restrict__ b_scales,
    int64_t bs_g, int64_t bs_c, const T* __restrict__ bias, int m, int n, int k, int64_t lda, int64_t ldb,
    int64_t ldc, int ss_per_split) {
  constexpr int D = NT == 1 ? 4 : 3;   // ring of weight super-steps (32 NT + NT VGPRs each), D - 1 in flight
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint4* a_img = reinterpret_cast<const uint4*>(smem);
  uint32_t* as_lds = reinterpret_cast<uint32_t*>(smem + (size_t)ss_per_split * MT * kF8eImgBytes);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lc = lane & 15, lr = lane >> 4;
  const int total_steps = k >> 7;
  const int total_ss = (total_steps + 3) >> 2;
  const int ss0 = blockIdx.y * ss_per_split;
  const int nss = min(ss_per_split, total_ss - ss0);
  // lines (k-steps) of this range's last super-step (4 unless it is the ragged end of K): lines >= r are zeroed in
  // the activation image; the lanes that would read them re-read line 0 (in range) of the weights and their scales
  const int r = min(4, total_steps - (ss0 + nss - 1) * 4);
  const int n0 = (blockIdx.x * 4 + wave) * (16 * NT);
  const uint8_t* b_src[NT];
  const uint8_t* bs_src[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    int col = n0 + NT * lc + t;
    col = col < n ? col : n - 1;
    b_src[t] = b + (int64_t)col * ldb + (int64_t)ss0 * 512 + 16 * (lr & 1);
    if constexpr (MX) bs_src[t] = b_scales + (int64_t)col * bs_c + ss0 * 16;
    else bs_src[t] = b_scales + (int64_t)(col >> 7) * bs_c + (int64_t)(ss0 * 4) * bs_g;
  }
  uint4 bq[D][NT][8];
  uint32_t bsc[D][NT];
  auto load_b = [&](int kk, uint4 (&dst)[NT][8], uint32_t (&dsc)[NT]) {
    const int kc = kk < nss ? kk : nss - 1;   // (clamped, not branched: beyond the range the last step is re-read)
    const int lim = kc == nss - 1 ? r : 4;    // lines (k-steps) of this super-step; a line beyond re-reads line 0
    const int l0 = (lr >> 1) < lim ? (lr >> 1) : 0, l1 = 2 + (lr >> 1) < lim ? 2 + (lr >> 1) : 0;
    const int lsc = kc * 4 + (lr < lim ? lr : 0);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const uint8_t* p0 = b_src[t] + (kc * 4 + l0) * 128;
      const uint8_t* p1 = b_src[t] + (kc * 4 + l1) * 128;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        dst[t][2 * s] = *reinterpret_cast<const uint4*>(p0 + 32 * s);
        dst[t][2 * s + 1] = *reinterpret_cast<const uint4*>(p1 + 32 * s);
      }
      if constexpr (MX) dsc[t] = *reinterpret_cast<const uint32_t*>(bs_src[t] + lsc * 4);
      else dsc[t] = bs_src[t][lsc * bs_g];
    }
  };
#pragma unroll
  for (int s = 0; s < D - 1; ++s) load_b(s, bq[s], bsc[s]);
  {
    // activation image: one copy = (k-step, row tile, row half): 8 rows x 128 bytes, lane -> (row, 16-byte chunk) with
    // the slot rotation of f8b_decode_kernel; the copies are dealt round-robin to the waves
    const uint32_t lds_base = __builtin_amdgcn_readfirstlane(lds_addr_of(smem));
    const int valid = (nss - 1) * 4 + r;
    const int copies = nss * 4 * MT * 2;
    const int rm_row = lane >> 3, rm_chunk = (lane & 7) ^ ((lane >> 3) & 6);
    for (int q = wave; q < copies; q += 4) {
      const int j = q & 1, i = (q >> 1) % MT, kst = (q >> 1) / MT;
      if (kst >= valid) {
        reinterpret_cast<uint4*>(smem)[q * 64 + lane] = make_uint4(0, 0, 0, 0);
        continue;
      }
      int row = 16 * i + 8 * j + rm_row;
      row = row < m ? row : m - 1;           // rows >= m only feed accumulator rows that are never stored
      lds_dma16(a + (int64_t)row * lda + (int64_t)(ss0 * 4 + kst) * 128 + 16 * rm_chunk, lds_base + q * 1024);
    }
    // scale bytes in read order: the dword (MX: groups 4 lr .. 4 lr + 3; block: the byte of k-step lr) of lane (lr, lc)
    for (int idx = threadIdx.x; idx < nss * MT * 64; idx += 256) {
      const int kk = idx / (MT * 64);
      const int rest = idx - kk * (MT * 64);
      const int lrq = (rest >> 4) & 3;
      int row = 16 * (rest >> 6) + (rest & 15);
      row = row < m ? row : m - 1;
      uint32_t v = 0x7f7f7f7fu;
      if (!(kk == nss - 1 && lrq >= r)) {
        if constexpr (MX) v = *reinterpret_cast<const uint32_t*>(a_scales + (int64_t)row * as_row + (ss0 + kk) * 16 + 4 * lrq);
        else v = a_scales[(int64_t)row * as_row + (int64_t)((ss0 + kk) * 4 + lrq) * as_g];
      }
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
  const int a_row = (lc >> 3) * 64 + 8 * (lc & 7), sw = lc & 6;   // chunk c of row lc sits in slot c ^ sw
  auto mma = [&](int kk, uint4 (&cur)[NT][8], uint32_t (&csc)[NT]) {
    const uint4* ap = a_img + ((kk * 4 + (lr >> 1)) * MT) * 128 + a_row;   // line lr >> 1; + 2 MT * 128: line 2 + (lr >> 1)
    uint32_t asc[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) asc[i] = as_lds[(kk * MT + i) * 64 + lane];
#define F8E_STEP(S)                                                                                       \
  _Pragma("unroll") for (int i = 0; i < MT; ++i) {                                                        \
    const uint4 a0 = ap[i * 128 + ((2 * (S) + (lr & 1)) ^ sw)];                                           \
    const uint4 a1 = ap[(2 * MT + i) * 128 + ((2 * (S) + (lr & 1)) ^ sw)];                                \
    _Pragma("unroll") for (int t = 0; t < NT; ++t)                                                        \
        acc[i][t] = f8e_mfma<MX ? (S) : 0>(a0, a1, cur[t][2 * (S)], cur[t][2 * (S) + 1], acc[i][t], asc[i], \
                                           csc[t]);                                                       \
  }
    F8E_STEP(0)
    F8E_STEP(1)
    F8E_STEP(2)
    F8E_STEP(3)
#undef F8E_STEP
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
constexpr int kF8ePiece = 2 * 16 * 64;          // uint4 per row half: 16 A + 16 B half tiles of 8 rows x 128 bytes
constexpr int kF8eStage = 2 * kF8ePiece;        // 64 KiB: 256 rows + 256 columns of 128 k
constexpr int kF8eScaleWords = 512;             // per stage: [A rows | B columns (MX) or the 2 column blocks] dwords
constexpr size_t kF8eTileLds = (size_t)2 * kF8eStage * 16 + 2 * kF8eScaleWords * 4;

template <typename T, bool MX>
__global__ __launch_bounds__(512, 2) void f8e_tile_kernel(
    T* __restrict__ out, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
    const uint8_t* __restrict__ a_scales, int64_t as_row, int64_t as_g, const uint8_t* __restrict__ b_scales,
    int64_t bs_g, int64_t bs_c, const T* __restrict__ bias, int m, int n, int k, int64_t lda, int64_t ldb,
    int64_t ldc, int num_m_blocks, int num_tiles, float* __restrict__ slabs, int sk) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint4* lds = reinterpret_cast<const uint4*>(smem);
  const uint8_t* sc_lds = reinterpret_cast<const uint8_t*>(smem + (size_t)2 * kF8eStage * 16);
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
  const int kstages_all = k >> 7;
  const int per_split = (kstages_all + sk - 1) / sk;
  const int ks0 = split * per_split;
  const int kstages = max(0, min(per_split, kstages_all - ks0));

  // operands in place: lane -> (row of a half tile, 16-byte chunk of the stage's 128 k bytes), slot rotation as in
  // f8b_tile_kernel; weight piece 4 G + t holds columns 64 G + 4 r + t, so a lane ends up with 4 adjacent outputs
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
  // scale copies into dword slot wave * 64 + lane.  MX: waves 0-3 the group dwords of 64 rows each, waves 4-7 of 64
  // columns each.  Block: waves 0-3 the aligned dword around a_s[row, k-step], wave 4 around the b_s of the tile's two
  // column blocks (slots 256, 257)
  const int nblk = (n + 127) >> 7;
  uintptr_t sc_src;
  int64_t sc_step;
  {
    int row = mb * 256 + (wave & 3) * 64 + lane;
    row = row < m ? row : m - 1;
    int col = nb * 256 + (wave & 3) * 64 + lane;
    col = col < n ? col : n - 1;
    const int cb = min(nb * 2 + (lane & 1), nblk - 1);
    if constexpr (MX) {
      sc_src = reinterpret_cast<uintptr_t>(wave < 4 ? a_scales + (int64_t)row * as_row : b_scales + (int64_t)col * bs_c);
      sc_step = 4;
    } else {
      sc_src = reinterpret_cast<uintptr_t>(wave < 4 ? a_scales + (int64_t)row * as_row : b_scales + (int64_t)cb * bs_c);
      sc_step = wave < 4 ? as_g : bs_g;
    }
  }
  // where this lane's scale bytes sit in the stage's dwords.  MX: byte lr (its group).  Block: the low address bits of
  // the byte — those of its 8 rows at k-step 0 packed 2 bits each, the k-step's share added per stage
  uint32_t a_low = 0;
  uintptr_t b_low_base = 0;
  if constexpr (!MX) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      int row = mb * 256 + wm * 128 + i * 16 + lc;
      row = row < m ? row : m - 1;
      a_low |= (uint32_t)((reinterpret_cast<uintptr_t>(a_scales) + (uintptr_t)((int64_t)row * as_row)) & 3) << (2 * i);
    }
    b_low_base = reinterpret_cast<uintptr_t>(b_scales) + (uintptr_t)((int64_t)min(nb * 2 + (wn >> 1), nblk - 1) * bs_c);
  }
  const uint32_t lds_base = __builtin_amdgcn_readfirstlane(lds_addr_of(smem));
  const uint32_t sc_base = lds_base + 2 * kF8eStage * 16;
  auto stage = [&](int buf, int ks) {
    const int64_t koff = (int64_t)(ks0 + ks) * 128;
#pragma unroll
    for (int pp = 0; pp < 2; ++pp) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int dst = buf * kF8eStage + pp * kF8ePiece + (wave * 2 + i) * 64;
        lds_dma16(a_src[i][pp] + koff, lds_base + dst * 16);
        lds_dma16(b_src[i][pp] + koff, lds_base + (dst + kBOff) * 16);
      }
    }
    if (MX || wave < 5) {
      const uintptr_t p = sc_src + (uintptr_t)((ks0 + ks) * sc_step);
      f8e_lds_dma4(reinterpret_cast<const void*>(p & ~(uintptr_t)3), sc_base + (buf * kF8eScaleWords + wave * 64) * 4);
    }
  };

  f32x4_t acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[i][t] = f32x4_t{0, 0, 0, 0};
  }
  // chunks lr and 4 + lr of row lc: the operand layout of the MFMA (see the head of the file)
  const int frag0 = (lc >> 3) * kF8ePiece + 8 * (lc & 7) + (lr ^ (lc & 6));
  const int frag1 = frag0 ^ 4;
  int cur = 0;
  if (kstages > 0) stage(0, 0);
  for (int ks = 0; ks < kstages; ++ks) {
    lds_dma_wait<0>();
    __syncthreads();
    if (ks + 1 < kstages) stage(cur ^ 1, ks + 1);    // (slot cur ^ 1: its readers passed the barrier above)
    const uint4* abuf = lds + cur * kF8eStage + (wm * 8) * 64;
    const uint4* bbuf = lds + cur * kF8eStage + kBOff + (wn * 4) * 64;
    const uint8_t* sa = sc_lds + (cur * kF8eScaleWords + wm * 128 + lc) * 4;
    const uint8_t* sb = sc_lds + (cur * kF8eScaleWords + 256) * 4;
    uint32_t a_off = 0;   // MX: unused
    if constexpr (MX) {
      sa += lr;
      sb += (wn * 64 + 4 * lc) * 4 + lr;
    } else {
      a_off = (uint32_t)((ks0 + ks) * as_g);
      sb += (wn >> 1) * 4 + ((b_low_base + (uintptr_t)((ks0 + ks) * bs_g)) & 3);
    }
    uint4 bf[4][2];
    uint32_t bs[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      bf[t][0] = bbuf[t * 64 + frag0];
      bf[t][1] = bbuf[t * 64 + frag1];
      bs[t] = MX ? sb[t * 4] : sb[0];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint4 a0 = abuf[i * 64 + frag0], a1 = abuf[i * 64 + frag1];
      const uint32_t as = MX ? sa[i * 64] : sa[i * 64 + (((a_low >> (2 * i)) + a_off) & 3)];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[i][t] = f8e_mfma<0>(a0, a1, bf[t][0], bf[t][1], acc[i][t], as, bs[t]);
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
__global__ __launch_bounds__(256) void f8e_finish_kernel(T* __restrict__ out, const float* __restrict__ ws,
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
static int f8e_launch_finish(const F8eArgs& g, int sk) {
  f8e_route_mask |= MI355X_F8E_ROUTE_SUM_SLABS;
  const int64_t threads = (int64_t)g.m * (g.n / 4);
  hipLaunchKernelGGL((f8e_finish_kernel<T>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, g.stream,
                     static_cast<T*>(g.out), g.ws, static_cast<const T*>(g.bias), g.m, g.n, g.ldc, sk);
  return check_launch("scaled_mm_fp8_e8m0(finish)");
}

// plan of the stream kernel: the cost model of plan_block_decode (fp8_block_gemm.hip, the same weight stream) in
// super-steps of 512 k: NT column tiles per wave (2 at most: the ring holds D super-steps of 33 VGPRs per column),
// sk <= 8 K splits (sum_slabs adds at most 8) of `ss` super-steps, the activation image of a split <= 128 KiB.
struct F8eStreamPlan {
  int nt, sk, ss;
};
static bool plan_f8e_stream(int m, int n, int k, int64_t ws_elems, F8eStreamPlan* p) {
  const int total = (k + 511) / 512;
  const int mt = m <= 16 ? 1 : (m <= 32 ? 2 : 4);
  const int max_ss = (128 * 1024) / (mt * kF8eImgBytes);
  double best = 1e30;
  bool found = false;
  for (int nt = 2; nt >= 1; nt >>= 1) {
    const int nblk = (n + 64 * nt - 1) / (64 * nt);
    for (int sk = 1; sk <= 8 && sk <= total; ++sk) {
      const int ss = (total + sk - 1) / sk;
      if ((total + ss - 1) / ss != sk || ss > max_ss) continue;
      if (sk > 1 && (int64_t)sk * m * n > ws_elems) continue;
      const int wgs = nblk * sk;
      const int img = mt * ss * (kF8eImgBytes + kF8eScBytes);
      const int reg_cu = nt == 2 ? 1 : 2;   // workgroups per CU the ring's VGPRs leave room for (244 / <= 206)
      int per_cu = (160 * 1024) / img;
      per_cu = per_cu < 1 ? 1 : (per_cu > reg_cu ? reg_cu : per_cu);
      const int rounds = (wgs + 256 * per_cu - 1) / (256 * per_cu);
      const int active = wgs < 256 ? wgs : 256;
      double rate = 6000.0 / active;              // GB/s per CU
      if (rate > 45.0) rate = 45.0;
      int conc = (wgs + 255) / 256;
      if (conc > per_cu) conc = per_cu;
      const double step_us = 4 * 8.2 * nt / rate * conc;
      double t = 5.5 + rounds * (img / 1024.0 / 68.0 + ss * step_us);
      if (sk > 1) t += 3.5 + 2.0 * (double)sk * m * n * 4 / 4e6;
      if (t < best) {
        best = t;
        *p = F8eStreamPlan{nt, sk, ss};
        found = true;
      }
    }
  }
  return found;
}

template <typename T, int MT, int NT, bool MX>
static int launch_f8e_stream(const F8eArgs& g, const F8eStreamPlan& p) {
  auto kern = f8e_stream_kernel<T, MT, NT, MX>;
  constexpr int kMaxLds = 144 * 1024;   // 128 KiB of image + its scales
  const size_t smem = (size_t)p.ss * MT * (kF8eImgBytes + kF8eScBytes);
  static PerDeviceOnce once;   // one per instantiation
  int dev;
  if (once.need(&dev)) {
    const hipError_t e =
        hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
    if (e != hipSuccess) {
      set_error("scaled_mm_fp8_e8m0(stream): cannot reserve %d B of LDS: %s", kMaxLds, hipGetErrorString(e));
      return MI355X_EUNSUPPORTED;
    }
    once.mark(dev);
  }
  f8e_route_mask |= MI355X_F8E_ROUTE_STREAM;
  const int nblk = (g.n + 64 * NT - 1) / (64 * NT);
  hipLaunchKernelGGL(kern, dim3(nblk, p.sk), dim3(256), smem, g.stream, static_cast<T*>(g.out), g.ws, g.a, g.b,
                     g.a_scales, g.as_row, g.as_g, g.b_scales, g.bs_g, g.bs_c, static_cast<const T*>(g.bias), g.m,
                     g.n, g.k, g.lda, g.ldb, g.ldc, p.ss);
  const int rc = check_launch("scaled_mm_fp8_e8m0(stream)");
  if (rc || p.sk == 1) return rc;
  return f8e_launch_finish<T>(g, p.sk);
}

// one pass of <= 64 rows
template <typename T, bool MX>
static int run_f8e_stream(const F8eArgs& g, const F8eStreamPlan& p) {
#define F8E_NT(MTV) (p.nt == 2 ? launch_f8e_stream<T, MTV, 2, MX>(g, p) : launch_f8e_stream<T, MTV, 1, MX>(g, p))
  if (g.m <= 16) return F8E_NT(1);
  if (g.m <= 32) return F8E_NT(2);
  return F8E_NT(4);
#undef F8E_NT
}

template <typename T, bool MX>
static int run_f8e_tile(const F8eArgs& g) {
  int sk = 1;
  if (g.ws != nullptr) sk = plan_tile_split(g.m, g.n, g.k / 128, g.ws_elems, 0);
  static PerDeviceOnce once;
  int dev;
  if (once.need(&dev)) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(f8e_tile_kernel<T, MX>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)kF8eTileLds);
    if (e != hipSuccess) {
      set_error("scaled_mm_fp8_e8m0(tile): cannot reserve %zu B of LDS: %s", kF8eTileLds, hipGetErrorString(e));
      return MI355X_EUNSUPPORTED;
    }
    once.mark(dev);
  }
  f8e_route_mask |= MI355X_F8E_ROUTE_TILE;
  const int num_m_blocks = (g.m + 255) / 256, num_n_blocks = (g.n + 255) / 256;
  const int num_tiles = num_m_blocks * num_n_blocks;
  hipLaunchKernelGGL((f8e_tile_kernel<T, MX>), dim3(num_tiles * sk), dim3(512), kF8eTileLds, g.stream,
                     static_cast<T*>(g.out), g.a, g.b, g.a_scales, g.as_row, g.as_g, g.b_scales, g.bs_g, g.bs_c,
                     static_cast<const T*>(g.bias), g.m, g.n, g.k, g.lda, g.ldb, g.ldc, num_m_blocks, num_tiles, g.ws,
                     sk);
  const int rc = check_launch("scaled_mm_fp8_e8m0(tile)");
  if (rc || sk == 1) return rc;
  return f8e_launch_finish<T>(g, sk);
}

// Router.  m <= 65: passes of 64 rows through the stream kernel, above: the tile kernel.  The fp32 block path switches
// at 320, but this tile kernel with its K split overtakes a SECOND stream pass on three of the four Llama-3-70B TP = 8
// shapes (forced either way, profiles/fp8_e8m0_gemm.txt: at m = 128 the tile kernel takes 21.5 / 26.9 / 21.9 us
// against 22.3 / 43.8 / 32.5 us of two passes; only the k = 1024 shape keeps the passes ahead, 14.7 against 17.1 us, up
// to m = 128); m = 65 keeps the two-pass form (64 rows + 1) alive and tested, as on the MX-FP4 path.
// MI355X_F8E_TILE_MIN_M for A/B runs.  A shape the stream kernel has no plan for (a K range too long for LDS and no
// workspace to split it) goes to the tile kernel whatever m is.
static int f8e_tile_min_m() {
  static const int v = [] { const char* e = getenv("MI355X_F8E_TILE_MIN_M"); return e ? atoi(e) : 66; }();
  return v;
}

template <typename T, bool MX>
static int run_f8e(const F8eArgs& g) {
  if (g.m < f8e_tile_min_m()) {
    F8eStreamPlan plans[2];   // full passes, the ragged last one
    const int tail = g.m % 64;
    bool ok = true;
    if (g.m >= 64) ok = plan_f8e_stream(64, g.n, g.k, g.ws_elems, &plans[0]);
    if (ok && tail) ok = plan_f8e_stream(tail, g.n, g.k, g.ws_elems, &plans[1]);
    if (ok) {
      for (int row0 = 0; row0 < g.m; row0 += 64) {
        F8eArgs p = g;
        p.m = g.m - row0 < 64 ? g.m - row0 : 64;
        p.a = g.a + (int64_t)row0 * g.lda;
        p.out = static_cast<T*>(g.out) + (int64_t)row0 * g.ldc;
        p.a_scales = g.a_scales + (int64_t)row0 * g.as_row;
        const int rc = run_f8e_stream<T, MX>(p, plans[p.m == 64 ? 0 : 1]);
        if (rc) return rc;
      }
      return MI355X_OK;
    }
  }
  return run_f8e_tile<T, MX>(g);
}

}  // namespace mi355x

using namespace mi355x;

extern "C" int mi355x_scaled_mm_fp8_e8m0_last_route(void) { return f8e_route_mask; }

extern "C" int64_t mi355x_scaled_mm_fp8_e8m0_workspace_elems(int m, int n, int k) {
  if (m <= 0 || n <= 0 || k <= 0 || k % 128 != 0) return 0;
  if (m < f8e_tile_min_m()) return (int64_t)8 * (m < 64 ? m : 64) * n;
  const int sk = plan_tile_split(m, n, k / 128, INT64_MAX, 0);
  return sk > 1 ? (int64_t)sk * m * n : 0;
}

extern "C" int mi355x_scaled_mm_fp8_e8m0(void* out, const void* a, const void* b, const void* a_scales,
                                         int64_t a_s_stride0, int64_t a_s_stride1, const void* b_scales,
                                         int64_t b_s_stride0, int64_t b_s_stride1, const void* bias, float* workspace,
                                         int64_t workspace_elems, int m, int n, int k, int scale_group, int64_t lda,
                                         int64_t ldb, int64_t ldc, int out_dtype, mi355x_stream stream) {
  f8e_route_mask = 0;
  MI355X_REQUIRE(m >= 0 && n > 0 && k > 0, MI355X_EINVAL, "scaled_mm_fp8_e8m0: bad sizes");
  MI355X_REQUIRE(scale_group == 32 || scale_group == 128, MI355X_EUNSUPPORTED,
                 "scaled_mm_fp8_e8m0: scale_group = %d, only 32 (MX) and 128 (block) are supported", scale_group);
  MI355X_REQUIRE(k % 128 == 0, MI355X_EUNSUPPORTED, "scaled_mm_fp8_e8m0: k = %d must be a multiple of 128", k);
  MI355X_REQUIRE(n % 16 == 0, MI355X_EUNSUPPORTED, "scaled_mm_fp8_e8m0: n = %d must be a multiple of 16", n);
  MI355X_REQUIRE(lda % 16 == 0 && ldb % 16 == 0 && lda >= k && ldb >= k, MI355X_EUNSUPPORTED,
                 "scaled_mm_fp8_e8m0: lda / ldb must be multiples of 16 bytes, >= k");
  MI355X_REQUIRE(ldc % 8 == 0 && ldc >= n, MI355X_EUNSUPPORTED,
                 "scaled_mm_fp8_e8m0: rows of out must be multiples of 16 bytes, >= n elements");
  MI355X_REQUIRE(a_s_stride0 >= 0 && a_s_stride1 >= 0 && b_s_stride0 >= 0 && b_s_stride1 >= 0, MI355X_EINVAL,
                 "scaled_mm_fp8_e8m0: negative scale stride");
  const bool mx = scale_group == 32;
  if (mx) {
    MI355X_REQUIRE(a_s_stride1 == 1 && b_s_stride0 == 1, MI355X_EUNSUPPORTED,
                   "scaled_mm_fp8_e8m0: MX scales must be contiguous along the K groups");
    MI355X_REQUIRE(a_s_stride0 % 4 == 0 && b_s_stride1 % 4 == 0 && a_s_stride0 >= k / 32 && b_s_stride1 >= k / 32,
                   MI355X_EUNSUPPORTED, "scaled_mm_fp8_e8m0: MX scale rows must be multiples of 4 bytes, >= k / 32");
  }
  MI355X_REQUIRE(workspace_elems >= 0, MI355X_EINVAL, "scaled_mm_fp8_e8m0: negative workspace size");
  if (m == 0) return MI355X_OK;
  MI355X_REQUIRE(out && a && b && a_scales && b_scales, MI355X_EINVAL, "scaled_mm_fp8_e8m0: null pointer");
  MI355X_REQUIRE(((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) |
                   reinterpret_cast<uintptr_t>(out)) & 15) == 0,
                 MI355X_EUNSUPPORTED, "scaled_mm_fp8_e8m0: a, b and out must be 16-byte aligned");
  MI355X_REQUIRE(!mx || ((reinterpret_cast<uintptr_t>(a_scales) | reinterpret_cast<uintptr_t>(b_scales)) & 3) == 0,
                 MI355X_EUNSUPPORTED, "scaled_mm_fp8_e8m0: MX scales must be 4-byte aligned");
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) workspace = nullptr;   // slabs are stored 16 bytes at a time
  F8eArgs g{out, static_cast<const uint8_t*>(a), static_cast<const uint8_t*>(b),
            static_cast<const uint8_t*>(a_scales), a_s_stride0, a_s_stride1, static_cast<const uint8_t*>(b_scales),
            b_s_stride0, b_s_stride1, bias, workspace, workspace ? workspace_elems : 0, m, n, k, lda, ldb, ldc,
            static_cast<hipStream_t>(stream)};
  return MI355X_DISPATCH_HALF(out_dtype, [&] { return mx ? run_f8e<scalar_t, true>(g) : run_f8e<scalar_t, false>(g); });
}
