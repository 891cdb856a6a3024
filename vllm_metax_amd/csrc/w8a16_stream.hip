// w8a16_stream.hip — 8-bit GPTQ GEMM below 1024 rows: an MFMA kernel that streams the weights HBM -> VGPR.
//
// C[m, n] = A[m, k] . W with W[kk][col] = T(fma(float(q), s, -z s)), z = stored zero + 1 (1 .. 256, kept in
// fp32: it never wraps in a byte), s the group's scale; products of a 9-bit and an 11-bit number are exact in
// fp32, so the value is rounded once, to T — the arithmetic of w8a16_gemm_any_kernel.  fp32 accumulation on
// v_mfma_f32_16x16x32_{bf16,f16}.
//
// Layouts (GemmArgs): qweight [K/4][N] uint32, byte i of word (kk, col) = W[4 kk + i][col]; qzeros [K/g][N/4],
// byte i of word j = column 4 j + i; scales [K/g][N] of T.
//
// Fragment mapping.  A wave owns 64 columns.  For the k-step kt (32 k = 8 word rows) lane (lr, lc) loads the two
// uint4 at word rows 8 kt + 2 lr and 8 kt + 2 lr + 1, columns 64 G + 4 lc .. + 3: a wave instruction reads four
// contiguous 256-byte runs, whole cache lines.  Word t of the first load and word t of the second are the 8
// consecutive k (natural byte order) of column 64 G + 4 lc + t: the B fragment of the column-interleaved tile t
// (columns 64 G + 4 lc' + t, lc' = 0 .. 15).  So a lane's four accumulators of a row are four ADJACENT output
// columns (one 8-byte store, or one 16-byte slab store), its four zero points are one qzeros word and its four
// scales one 8-byte load.
//
// Work split.  A workgroup is 4 waves = NWC column groups of 64 x KW k-parts (NWC KW = 4, chosen per launch): wide
// shapes run 256 columns per workgroup (KW = 1), narrow ones (a TP rank's qkv) 64 columns with the workgroup's K
// range cut into four contiguous parts, added in part order through LDS at the end.  On top of that K is split
// across workgroups (grid.y <= 8) through fp32 slabs [sk][rows][n], added in slab order by
// w4a16_sum_slabs_kernel: no memset, no atomics, the result does not depend on timing and replays from a graph.
//
// Data movement.
//   * Weights: non-temporal 16-byte loads into a register ring of D = 6 k-steps (5 in flight per wave, 10 KiB);
//     the scale pair-of-words and the zero word of a step travel in the same ring entry (they hit L1/L2: a group
//     of 128 is re-read four times), so that a group change never waits on memory.  Loads past the wave's range
//     are clamped onto its last step, never branched around: the wait-count pass keeps counted vmcnt waits.
//   * Activations: the rows of the K range are copied row-major -> LDS by LDS-DMA with per-lane source addresses,
//     8 rows x 128 bytes (whole lines) per wave instruction, slot 8 (row & 7) + (chunk ^ (row & 6)) inside the
//     1-KiB copy — the rotation of gemm8_decode_kernel, which keeps the four ds_read_b128 lane groups of a
//     fragment read on distinct bank groups.  Rows >= m read row m - 1 again (the DMA cannot write zeros; they
//     only feed accumulator rows that are never stored).  The image holds at most 16 / MT stages of 128 k over all
//     k-parts (64 KiB at every MT: two workgroups per CU); a longer range is re-staged chunk by chunk between two
//     barriers.  No other barrier in the loop, no shared weight ring.
//   * Dequant: v_cvt_f32_ubyte0..3, plain v_fma_f32 (see dequant_word in w4a16.cuh), Mfma<T>::pack; scale and
//     -z s are refreshed when a k-step starts a group (groups are multiples of 32).
#include <stdio.h>
#include <stdlib.h>

#include "w4a16.cuh"

namespace mi355x {

namespace {

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint4 load_nt16(const u32x4_t* p) {
  const u32x4_t v = __builtin_nontemporal_load(p);
  return make_uint4(v.x, v.y, v.z, v.w);
}

// 8 consecutive k of one column (two words of 4 bytes) -> MFMA B fragment
template <typename T>
__device__ __forceinline__ uint4 dequant_bytes8(uint32_t lo, uint32_t hi, float s, float zs) {
  auto f = [&](float q) {
    float r;
    asm("v_fma_f32 %0, %1, %2, %3" : "=v"(r) : "v"(q), "v"(s), "v"(zs));
    return r;
  };
  uint4 r;
  r.x = Mfma<T>::pack(f(cvt_ubyte0(lo)), f(cvt_ubyte1(lo)));
  r.y = Mfma<T>::pack(f(cvt_ubyte2(lo)), f(cvt_ubyte3(lo)));
  r.z = Mfma<T>::pack(f(cvt_ubyte0(hi)), f(cvt_ubyte1(hi)));
  r.w = Mfma<T>::pack(f(cvt_ubyte2(hi)), f(cvt_ubyte3(hi)));
  return r;
}

struct StreamStage {   // one k-step (32 k) of a wave's 64 columns
  uint4 w0, w1;        // word rows 8 kt + 2 lr, + 1
  uint2 sc;            // 4 scales of T
  uint32_t z;          // 4 stored zero points
};

constexpr int kStreamRing = 6;

}  // namespace

// gsteps = group / 32; sps = 128-k stages per K split (grid.y); kw = k-parts per workgroup (1, 2, 4);
// csw = stages per k-part in one LDS image (dynamic LDS = kw * csw * MT * 4 KiB)
template <typename T, int MT>
__global__ __launch_bounds__(256) void w8a16_gemm_stream_kernel(
    T* __restrict__ c, float* __restrict__ slabs, const T* __restrict__ a, int64_t lda,
    const uint32_t* __restrict__ qw, const T* __restrict__ scales, const uint32_t* __restrict__ qz, int rows,
    int n, int k, int gsteps, int sps, int kw, int csw) {
  constexpr int D = kStreamRing;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint4* a_img = reinterpret_cast<const uint4*>(smem);   // [k-part][stage][64-k unit][row tile][row half][64]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lc = lane & 15, lr = lane >> 4;
  const int nwc = 4 / kw;
  const int cg = wave % nwc, kp = wave / nwc;
  const int total_stages = k >> 7;
  const int wg_s0 = blockIdx.y * sps;
  const int wg_ns = min(sps, total_stages - wg_s0);           // >= 1 (the planner leaves no empty split)
  const int spw = (wg_ns + kw - 1) / kw;                      // stages per k-part, the same for all waves
  const int w_off = min(kp * spw, wg_ns);
  const int w_ns = min(spw, wg_ns - w_off);                   // this wave's stages (0 for a part past the range)
  const int w_s0 = wg_s0 + min(w_off, wg_ns - 1);             // a valid stage even then
  const int nk = 4 * w_ns, nloop = 4 * spw;
  int n0 = (blockIdx.x * nwc + cg) * 64;
  const bool live = n0 < n;                                   // (n % 256 != 0: the last workgroup's spare waves)
  if (!live) n0 = n - 64;

  const int64_t n4 = n >> 2;
  const u32x4_t* wp =
      reinterpret_cast<const u32x4_t*>(qw) + ((int64_t)(w_s0 * 32 + 2 * lr) * n + n0 + 4 * lc) / 4;
  const T* sp = scales + n0 + 4 * lc;
  const uint32_t* zp = qz + (n0 >> 2) + lc;
  const int rem0 = (w_s0 * 4) % gsteps;
  int ld = 0, ld_gi = (w_s0 * 4) / gsteps, ld_rem = rem0;
  auto load = [&](StreamStage& st) {
    st.w0 = load_nt16(wp);
    st.w1 = load_nt16(wp + n4);
    st.sc = *reinterpret_cast<const uint2*>(sp + (int64_t)ld_gi * n);
    st.z = zp[(int64_t)ld_gi * n4];
    if (ld < nk - 1) {   // (clamped, not branched: beyond the range the last step is read again)
      ++ld;
      wp += 8 * n4;   // 8 word rows
      if (++ld_rem == gsteps) {
        ld_rem = 0;
        ++ld_gi;
      }
    }
  };

  const uint32_t lds_base = __builtin_amdgcn_readfirstlane(lds_addr_of(smem));
  const int rm_row = lane >> 3, rm_chunk = (lane & 7) ^ ((lane >> 3) & 6);
  // copy q = (((p * csw + s) * 2 + u) * MT + i) * 2 + j: rows 8 j .. 8 j + 7 of row tile i, the 64 k of unit u of
  // stage s of k-part p's chunk; dealt round-robin to the 4 waves
  auto stage_a = [&](int chunk) {
    const int copies = kw * csw * 4 * MT;
    for (int q = wave; q < copies; q += 4) {
      const int j = q & 1, i = (q >> 1) % MT, uu = (q >> 1) / MT;
      const int u = uu & 1, s = (uu >> 1) % csw, p = (uu >> 1) / csw;
      int st = wg_s0 + p * spw + chunk * csw + s;
      st = st < total_stages ? st : total_stages - 1;          // (past a part's range: bytes nobody reads)
      int row = 16 * i + 8 * j + rm_row;
      row = row < rows ? row : rows - 1;
      lds_dma16(a + (int64_t)row * lda + (int64_t)st * 128 + u * 64 + 8 * rm_chunk, lds_base + q * 1024);
    }
  };

  StreamStage ring[D];
  stage_a(0);
#pragma unroll
  for (int s = 0; s < D - 1; ++s) load(ring[s]);
  lds_dma_wait<0>();
  __syncthreads();

  f32x4_t acc[MT][4];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[i][t] = f32x4_t{0, 0, 0, 0};
  }
  float s4[4], zs4[4];
  auto refresh = [&](const StreamStage& st) {
    struct T4 {
      T v[4];
    };
    const T4 sv = __builtin_bit_cast(T4, st.sc);
    const float z[4] = {cvt_ubyte0(st.z), cvt_ubyte1(st.z), cvt_ubyte2(st.z), cvt_ubyte3(st.z)};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      s4[t] = to_f32(sv.v[t]);
      zs4[t] = -((z[t] + 1.0f) * s4[t]);   // z up to 256: exact (9 x 11 bits)
    }
  };
  // lane (lr, lc) of row tile i: row lc's 8 k of k-group lr — chunk 4 h + lr of the 64-k unit, h = step & 1
  const int a_frag = (lc >> 3) * 64 + 8 * (lc & 7) + (lr ^ (lc & 6));
  auto mma = [&](int cs, const StreamStage& st) {
    const uint4* ap = a_img + (kp * csw * 2 + (cs >> 1)) * (MT * 128) + (a_frag ^ ((cs & 1) << 2));
    uint4 af[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) af[i] = ap[i * 128];
    const uint32_t lo[4] = {st.w0.x, st.w0.y, st.w0.z, st.w0.w};
    const uint32_t hi[4] = {st.w1.x, st.w1.y, st.w1.z, st.w1.w};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const uint4 bf = dequant_bytes8<T>(lo[t], hi[t], s4[t], zs4[t]);
#pragma unroll
      for (int i = 0; i < MT; ++i) acc[i][t] = Mfma<T>::run(af[i], bf, acc[i][t]);
    }
  };
  int cs = 0, chunk = 0, crem = rem0;
  bool fresh = true;
  auto step = [&](int kk, const StreamStage& st) {
    if (cs == 4 * csw) {   // the image is used up: every wave has left it, the next chunk lands, every wave sees it
      __syncthreads();
      stage_a(++chunk);
      lds_dma_wait<0>();
      __syncthreads();
      cs = 0;
    }
    if (kk < nk) {
      if (fresh || crem == 0) refresh(st);
      fresh = false;
      mma(cs, st);
      if (++crem == gsteps) crem = 0;
    }
    ++cs;
  };
  int kk = 0;
  for (; kk + D <= nloop; kk += D) {
#pragma unroll
    for (int s = 0; s < D; ++s) {
      load(ring[(s + D - 1) % D]);
      __builtin_amdgcn_sched_barrier(0);
      step(kk + s, ring[s]);
    }
  }
  // the last nloop - kk < D steps are in flight or in registers: no further loads
#pragma unroll
  for (int s = 0; s < D - 1; ++s) {
    if (kk + s < nloop) step(kk + s, ring[s]);
  }

  if (kw > 1) {   // k-parts 1 .. kw - 1 hand their tiles to part 0 through LDS; added in part order
    float4* red = reinterpret_cast<float4*>(smem);
    __syncthreads();
    if (kp > 0) {
#pragma unroll
      for (int i = 0; i < MT; ++i) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const f32x4_t v = acc[i][t];
          red[((((kp - 1) * nwc + cg) * MT + i) * 4 + t) * 64 + lane] = make_float4(v[0], v[1], v[2], v[3]);
        }
      }
    }
    __syncthreads();
    if (kp == 0) {
      for (int p = 1; p < kw; ++p) {
#pragma unroll
        for (int i = 0; i < MT; ++i) {
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const float4 v = red[((((p - 1) * nwc + cg) * MT + i) * 4 + t) * 64 + lane];
            acc[i][t] += f32x4_t{v.x, v.y, v.z, v.w};
          }
        }
      }
    }
  }
  if (kp != 0 || !live) return;

  const int col0 = n0 + 4 * lc;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = 16 * i + 4 * lr + j;
      if (row >= rows) continue;
      if (gridDim.y == 1) {
        const uint2 v = make_uint2(Mfma<T>::pack(acc[i][0][j], acc[i][1][j]),
                                   Mfma<T>::pack(acc[i][2][j], acc[i][3][j]));
        *reinterpret_cast<uint2*>(c + (int64_t)row * n + col0) = v;
      } else {
        *reinterpret_cast<float4*>(slabs + ((int64_t)blockIdx.y * rows + row) * n + col0) =
            make_float4(acc[i][0][j], acc[i][1][j], acc[i][2][j], acc[i][3][j]);
      }
    }
  }
}

// ---- host side ------------------------------------------------------------------------------
namespace {

struct StreamPlan {
  int kw, sk, sps;   // k-parts per workgroup, K splits across workgroups, stages per split
  double est_us;
};

// stages of one k-part that fit the LDS image (<= 16 / MT stages of 128 k over all parts: 64 KiB)
int stream_chunk_stages(int mt, int kw, int sps) {
  const int spw = (sps + kw - 1) / kw;
  const int cap = 16 / (mt * kw) > 0 ? 16 / (mt * kw) : 1;
  return spw < cap ? spw : cap;
}

// Cost model (microseconds) behind the choice of k-parts and K split.  A wave's k-step (32 k x 64 columns, 2 KiB of
// weights) costs ~0.14 us of VALU issue on its SIMD (80 dequant instructions + the refresh) and, with 5 steps in
// flight against ~2 us of loaded HBM latency, at least ~0.4 us of a lone wave's time; the chip streams ~6.5 TB/s.
// A re-staged chunk costs a drain of the ring (~1 us); a workgroup's activation rows fill LDS at ~50 GB/s per CU
// (what separates 64-column from 128-column workgroups at equal steps per wave); the LDS add of the k-parts ~0.5 us;
// a K split one more launch (~1.5 us in a graph) and its slabs written and read back at ~3 TB/s (8 slabs of a
// 64 x 8192 pass cost more than they save at k = 1024).  K splits of 1, 2, 4 and 8: the set the sweep covers.
// Fitted to the sweep of scripts/bench_w8a16.py --sweep (profiles/w8a16_stream.txt).
StreamPlan plan_stream(int rows, int n, int k, int64_t ws_elems) {
  const int mt = rows <= 16 ? 1 : (rows <= 32 ? 2 : 4);
  const int stages = k / 128, cgn = n / 64;
  int fkw = 0, fsk = 0;
  if (const char* f = getenv("MI355X_W8_STREAM_FORCE")) {   // "kw,sk" (kernel experiments, the planner's sweep)
    if (sscanf(f, "%d,%d", &fkw, &fsk) != 2 || !(fkw == 1 || fkw == 2 || fkw == 4) || fsk < 1) fkw = fsk = 0;
    if (fsk > 8) fsk = 8;
    if (fsk > stages) fsk = stages;
    if (fsk > 1) {   // a split that is empty at its end or has no room runs unsplit
      const int sps = (stages + fsk - 1) / fsk;
      if ((stages + sps - 1) / sps != fsk || (int64_t)fsk * rows * n > ws_elems) fsk = 1;
    }
  }
  StreamPlan best{1, 1, stages, 1e30};
  for (int kw = 1; kw <= 4; kw *= 2) {
    if (fkw && kw != fkw) continue;
    const int wgx = (cgn * kw + 3) / 4;
    for (int sk = 1; sk <= 8; ++sk) {
      if (fsk ? sk != fsk : (sk & (sk - 1)) != 0) continue;
      const int sps = (stages + sk - 1) / sk;
      if ((stages + sps - 1) / sps != sk) continue;            // (an empty last split)
      if (sk > 1 && (int64_t)sk * rows * n > ws_elems) continue;
      const int spw = (sps + kw - 1) / kw;
      const int csw = stream_chunk_stages(mt, kw, sps);
      const int per_cu = (wgx * sk + 255) / 256;               // workgroups a CU runs, one wave per SIMD each
      const double valu = per_cu * 4.0 * spw * 0.14;
      const double lat = ((per_cu + 1) / 2) * 4.0 * spw * 0.4; // two workgroups resident per CU
      const double hbm = (double)n * k / 6.5e6;
      double t = valu > lat ? valu : lat;
      t = 3.0 + (t > hbm ? t : hbm) + 1.0 * ((spw + csw - 1) / csw - 1) * ((per_cu + 1) / 2);
      t += per_cu * (mt * 4096.0 * sps) / 50e3;                // the workgroup's activation rows, L2 -> LDS
      if (kw > 1) t += 0.5;
      if (sk > 1) t += 1.5 + 2.0 * ((double)sk * rows * n * 4) / 3e6;
      if (t < best.est_us) best = StreamPlan{kw, sk, sps, t};
    }
  }
  return best;
}

template <typename T, int MT>
int launch_stream(const GemmArgs& g, const T* a, T* c, int rows, const StreamPlan& p) {
  auto kern = w8a16_gemm_stream_kernel<T, MT>;
  static PerDeviceOnce attr_once;  // one per instantiation, one bit per device
  int dev;
  if (attr_once.need(&dev)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
    if (e != hipSuccess) {
      set_error("w8a16_gemm_stream: cannot reserve 64 KiB of LDS: %s", hipGetErrorString(e));
      return MI355X_EUNSUPPORTED;
    }
    attr_once.mark(dev);
  }
  const int csw = stream_chunk_stages(MT, p.kw, p.sps);
  const size_t lds = (size_t)p.kw * csw * MT * 4096;
  const int wgx = (g.n / 64 * p.kw + 3) / 4;
  hipLaunchKernelGGL(kern, dim3(wgx, p.sk), dim3(256), lds, g.stream, c, g.ws, a, g.lda, g.qw,
                     static_cast<const T*>(g.scales), g.qz, rows, g.n, g.k, g.group / 32, p.sps, p.kw, csw);
  w4_route_note(MI355X_W8_ROUTE_STREAM);
  return check_launch("w8a16_gemm_stream");
}

// returns 1 when the shape is not one this kernel takes (the caller falls back)
template <typename T>
int run_stream(const GemmArgs& g, int row0, int rows) {
  if (g.bits != 8 || g.zmode != kZeroGptq || rows < 1 || rows > 64 || g.n % 64 != 0 || g.k % 128 != 0 ||
      g.group % 32 != 0 || g.k % g.group != 0)
    return 1;
  if (g.fuse_silu || g.defer_sk != nullptr || g.a_packed || g.b_image != nullptr) return 1;
  if ((reinterpret_cast<uintptr_t>(g.qw) & 15) || (reinterpret_cast<uintptr_t>(g.scales) & 7) ||
      (reinterpret_cast<uintptr_t>(g.c) & 7))
    return 1;
  // (the slabs are stored 16 bytes at a time: a workspace that is not aligned so gets no K split)
  const bool ws_ok = g.ws != nullptr && (reinterpret_cast<uintptr_t>(g.ws) & 15) == 0;
  const T* a = static_cast<const T*>(g.a) + (int64_t)row0 * g.lda;
  T* c = static_cast<T*>(g.c) + (int64_t)row0 * g.n;
  const StreamPlan p = plan_stream(rows, g.n, g.k, ws_ok ? g.ws_elems : 0);
  int rc = rows <= 16 ? launch_stream<T, 1>(g, a, c, rows, p)
                      : (rows <= 32 ? launch_stream<T, 2>(g, a, c, rows, p) : launch_stream<T, 4>(g, a, c, rows, p));
  if (rc) return rc;
  if (p.sk > 1) {
    const int64_t q4 = (int64_t)rows * g.n / 4;
    hipLaunchKernelGGL(w4a16_sum_slabs_kernel<T>, dim3((q4 + 255) / 256), dim3(256), 0, g.stream, c, g.ws, q4,
                       p.sk);
    w4_route_note(MI355X_W4_ROUTE_SUM_SLABS);
    rc = check_launch("w4a16_sum_slabs");
  }
  return rc;
}

}  // namespace

int w8a16_gemm_stream_dispatch(const GemmArgs& g, int dtype, int row0, int rows) {
  if (dtype == MI355X_BF16) return run_stream<bf16_t>(g, row0, rows);
  if (dtype == MI355X_F16) return run_stream<f16_t>(g, row0, rows);
  return 1;
}

}  // namespace mi355x
