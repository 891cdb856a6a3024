// prefill_attention_hd.hip — the MFMA paged prefill / chunked-prefill kernel for head sizes 64 and 256
// (block_size 16, f16 / bf16, cache auto / fp8 e4m3 / fp8 e5m2; causal bottom-right, context > 0, GQA, varlen;
// sliding window and soft-cap in the OPTS instantiation).  ALiBi, the operand-image output and in-kernel rotary
// stay with head size 128 (prefill_attention.hip); every other shape stays on the general kernel there.
//
// Same formulation as the d128 kernel: S^T = K.Q^T with v_mfma_f32_16x16x32 (keys on rows, one query column per
// lane), the exponentiated, rounded scores ARE the B operand of O^T = V^T.P^T, online softmax with one rescale
// factor per lane and column tile, K / V blocks copied verbatim global -> LDS by LDS-DMA into a 3-slot ring with
// counted waits, key blocks past seq_len clamped and their V entries zeroed in LDS, heaviest query blocks first.
// What changes with the head size is the schedule:
//   * a K block [HD/8][16][8] / V block [HD][16] is HD * 32 bytes (HD * 16 for fp8): 2 KiB at 64, 8 KiB at 256;
//   * HD = 64: a stage is 64 keys (4 K + 4 V blocks, 16 KiB) — one barrier, one wait and ONE softmax pass (one
//     max reduction, one rescale of the accumulators) per 64 keys, then two 32-key PV steps; a 32-key stage would
//     have carried half the MFMAs of the d128 stage behind the same fixed cost.  Ring 48 KiB, 2+ workgroups per
//     CU.  Four waves with two 16-row query tiles each (QT = 2, 128 query rows per workgroup): every K / V
//     fragment read from LDS feeds two MFMAs.  Grids below 512 such workgroups take one tile per wave (QT = 1, 64
//     rows, twice the workgroups), as the d128 launcher does: measured 6 - 18 % faster at 128 - 256 workgroups,
//     up to 43 % slower at 512 and more (profiles/prefill_attn_head_sizes.txt).
//   * HD = 256: a stage is 32 keys (2 K + 2 V blocks, 32 KiB), ring 96 KiB: one workgroup per CU, and the kernel
//     is built for that (__launch_bounds__(512, 1)): EIGHT waves with one query tile each (NW = 8, QT = 1, 128
//     query rows per workgroup; 64 accumulator + 32 query-fragment registers of 160 VGPRs).  Two waves per SIMD let
//     one wave's softmax run under the other's MFMAs; four waves with two tiles each (252 VGPRs + 148 AGPRs of
//     the unified file, one wave per SIMD) read each fragment half as often but had nothing to overlap with and
//     measured 24 - 30 % slower at every shape.
#include "prefill_attention.cuh"

namespace mi355x {

constexpr int kHdStages = 3;   // LDS ring depth

template <int HD, bool KV8, int NW = 4>
struct HdShape {
  static constexpr int kNB = HD == 64 ? 4 : 2;               // cache blocks (16 keys) per stage
  static constexpr int kKeys = 16 * kNB;                     // keys per stage
  static constexpr int kBlkBytes = HD * 16 * (KV8 ? 1 : 2);  // one K or V block
  static constexpr int kStageBytes = 2 * kNB * kBlkBytes;    // [K blocks | V blocks]
  static constexpr int kCopies = kStageBytes / (1024 * NW);   // 1-KiB DMA pieces per wave and stage
  static constexpr int kSmem = kHdStages * kStageBytes;
};

template <typename T, int HD, bool KV8, bool OPTS, bool E5M2, int QT = 2, int NW = 4>
__global__ __launch_bounds__(64 * NW, HD == 256 ? 1 : 2) void paged_prefill_hd_kernel(
    T* __restrict__ out, const T* __restrict__ q, const void* __restrict__ k_cache_v,
    const void* __restrict__ v_cache_v, int num_heads, int num_kv_heads, float scale,
    const int* __restrict__ block_tables, const int* __restrict__ seq_lens,
    const int* __restrict__ cu_seqlens_q, int max_num_blocks_per_seq, int q_blocks_per_seq,
    int64_t q_stride, int64_t out_stride, int64_t kv_block_stride, int64_t kv_head_stride,
    const float* __restrict__ k_scale, const float* __restrict__ v_scale, int window, float softcap) {
  static_assert(HD == 64 || HD == 256, "head sizes of this kernel");
  using S = HdShape<HD, KV8, NW>;
  constexpr int kNB = S::kNB, kKeys = S::kKeys, kBlkBytes = S::kBlkBytes, kStageBytes = S::kStageBytes;
  constexpr int kCopies = S::kCopies;
  constexpr int kDS = HD / 32;   // QK MFMAs (32 head dims each) per key block and query tile
  constexpr int kDT = HD / 16;   // 16-row tiles of O^T
  constexpr int kNV = 4 * kNB;   // scores of one query column a lane holds per stage
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const char* k_cache = static_cast<const char*>(k_cache_v);   // strides below are in cache elements
  const char* v_cache = static_cast<const char*>(v_cache_v);
  constexpr int kCe = KV8 ? 1 : (int)sizeof(T);                // bytes per cache element
  if constexpr (KV8) scale *= *k_scale;

  // heaviest query blocks first (1-D grid: block = (reversed query block, head, sequence), sequence fastest)
  const int num_seqs_g = (int)gridDim.x / (q_blocks_per_seq * num_heads);
  const int per_qb = num_heads * num_seqs_g;
  const int qb = q_blocks_per_seq - 1 - (int)blockIdx.x / per_qb;
  const int rem = (int)blockIdx.x - (q_blocks_per_seq - 1 - qb) * per_qb;
  const int head = rem / num_seqs_g;
  const int seq = rem - head * num_seqs_g;
  const int q_begin = cu_seqlens_q[seq];
  const int q_len = cu_seqlens_q[seq + 1] - q_begin;
  constexpr int kQTile = 16 * NW * QT;   // query rows per workgroup
  const int m0 = qb * kQTile;
  if (m0 >= q_len) return;
  const int seq_len = seq_lens[seq];
  const int ctx = seq_len - q_len;
  const int kv_head = head / (num_heads / num_kv_heads);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lc = lane & 15;
  const int lr = lane >> 4;

  // ---- Q^T B-operand fragments: qf[qt][ds] = Q[row][32*ds + 8*lr .. +7] ----------------
  uint4 qf[QT][kDS];
  int qrow[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    qrow[qt] = m0 + wave * (16 * QT) + qt * 16 + lc;
    const int r = qrow[qt] < q_len ? qrow[qt] : q_len - 1;
    const T* qp = q + (int64_t)(q_begin + r) * q_stride + (int64_t)head * HD + 8 * lr;
#pragma unroll
    for (int ds = 0; ds < kDS; ++ds) qf[qt][ds] = *reinterpret_cast<const uint4*>(qp + 32 * ds);
  }

  f32x4_t oacc[QT][kDT];
  float mrun[QT], lrun[QT];    // (lrun: per-lane partial sums, its own keys only)
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
#pragma unroll
    for (int dt = 0; dt < kDT; ++dt) oacc[qt][dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    mrun[qt] = kNegBig;
    lrun[qt] = 0.f;
  }

  // keys needed by this workgroup: [0, kv_end)
  const int kv_end = min(seq_len, ctx + m0 + kQTile);
  const int num_tiles = (kv_end + kKeys - 1) / kKeys;
  const int* block_table = block_tables + (int64_t)seq * max_num_blocks_per_seq;
  const int num_seq_blocks = (seq_len + 15) / 16;

  // staging: a stage image is [K blk 0 .. kNB-1 | V blk 0 .. kNB-1], every block copied verbatim, cut into 1-KiB
  // pieces (one LDS-DMA instruction of one wave each); wave w copies pieces w, w + NW, ... of the stage
  const uint32_t lds_base = __builtin_amdgcn_readfirstlane(lds_addr_of(smem));
  // block ids of the sequence: 64 at a time in one VGPR, read back with readlane
  int bt_reg = 0;
  int bt_base = -64;
  auto block_id = [&](int blk) {
    if (blk >= bt_base + 64 || blk < bt_base) {
      bt_base = blk & ~63;
      const int i = bt_base + lane;
      bt_reg = block_table[i < num_seq_blocks ? i : num_seq_blocks - 1];
    }
    return (int64_t)__builtin_amdgcn_readlane(bt_reg, blk - bt_base);
  };
  auto stage_issue = [&](int slot, int tile) {
    constexpr int kPerBlk = kBlkBytes / 1024;   // pieces of one block
#pragma unroll
    for (int i = 0; i < kCopies; ++i) {
      const int piece = wave + NW * i;
      const int b = piece / kPerBlk;            // 0 .. kNB-1: K blocks, kNB .. 2 kNB-1: V blocks
      int blk = tile * kNB + (b < kNB ? b : b - kNB);
      blk = blk < num_seq_blocks ? blk : num_seq_blocks - 1;
      const int64_t pb = block_id(blk);
      const char* base = (b < kNB ? k_cache : v_cache) +
                         (pb * kv_block_stride + (int64_t)kv_head * kv_head_stride) * kCe;
      lds_dma16(base + (piece % kPerBlk) * 1024 + lane * 16, lds_base + slot * kStageBytes + piece * 1024);
    }
  };

  // sliding window: no row of this workgroup sees a key below (first query position) - W + 1
  int tile0 = 0;
  if constexpr (OPTS) {
    if (window > 0) tile0 = max(ctx + m0 - window + 1, 0) / kKeys;
  }
  stage_issue(0, tile0);
  if (tile0 + 1 < num_tiles) stage_issue(1, tile0 + 1);

  // softmax scale in log2 units; with OPTS the scores are brought to scaled units first (the cap acts there)
  const float sl2 = (OPTS ? 1.0f : scale) * 1.4426950408889634f;
  float cap_inv2 = 0.f;
  int wave_first = 0;   // first key any row of this wave may see
  if constexpr (OPTS) {
    if (softcap > 0.f) cap_inv2 = 2.0f * 1.4426950408889634f / softcap;   // tanh(x / cap) via 2^(2 x log2e / cap)
    if (window > 0) wave_first = ctx + m0 + wave * (16 * QT) - window + 1;
  }
  // every key <= this index is visible to EVERY query row of the wave (and is a real key)
  const int wave_limit_lo = min(ctx + m0 + wave * (16 * QT), seq_len - 1);
  const int wave_q_hi = ctx + m0 + wave * (16 * QT) + 16 * QT - 1;  // last key any row of this wave may see

  int cur = 0;   // ring slot of `tile`
  for (int tile = tile0; tile < num_tiles; ++tile) {
    // stage `tile` has landed once only the copies of the next stage are pending
    if (tile + 1 < num_tiles) lds_dma_wait<kCopies>();
    else lds_dma_wait<0>();
    __syncthreads();   // everybody's share of stage `tile` is in LDS; stage tile-1 is dead
    if (tile + 2 < num_tiles) {
      int slot = cur + 2;
      slot = slot >= kHdStages ? slot - kHdStages : slot;
      stage_issue(slot, tile + 2);
    }

    const int t0 = tile * kKeys;
    char* sbuf = smem + cur * kStageBytes;   // stage image
    if (t0 + kKeys > seq_len) {
      // last stage of the sequence: zero the V entries of keys >= seq_len once, in LDS (their probabilities are
      // exactly 0, and 0 * NaN must not reach O).  The kNB * HD rows of the V blocks go round the threads.
#pragma unroll
      for (int r = tid; r < kNB * HD; r += 64 * NW) {
        const int bi = r / HD;
        const int kvalid = seq_len - (t0 + 16 * bi);          // keys [0, kvalid) of this block are real
        uint32_t* vrow = reinterpret_cast<uint32_t*>(sbuf + kNB * kBlkBytes + r * (KV8 ? 16 : 32));
        if constexpr (!KV8) {
#pragma unroll
          for (int w = 0; w < 8; ++w) {
            if (2 * w >= kvalid) vrow[w] = 0u;
            else if (2 * w + 1 >= kvalid) vrow[w] &= 0xFFFFu;
          }
        } else {
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            const int live = kvalid - 4 * w;                    // live bytes of this dword
            if (live <= 0) vrow[w] = 0u;
            else if (live < 4) vrow[w] &= (1u << (8 * live)) - 1u;
          }
        }
      }
      __syncthreads();
    }
    if (t0 <= wave_q_hi && (!OPTS || t0 + kKeys > wave_first)) {
      // ---- S^T tiles: s[b][qt] = K_b . Q_qt^T, rows = keys 16*b + 4*lr + j, col = query lc
      f32x4_t s[kNB][QT];
#pragma unroll
      for (int b = 0; b < kNB; ++b) {
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) s[b][qt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ds = 0; ds < kDS; ++ds) {
          uint4 kf;
          if constexpr (!KV8) {
            // chunk 4 ds + lr, token lc of [HD/8][16][8]: lane-linear 16-byte reads
            kf = reinterpret_cast<const uint4*>(sbuf + b * kBlkBytes)[ds * 64 + lane];
          } else {
            // d = 32 ds + 8 lr + j -> 16-byte chunk 2 ds + (lr >> 1), bytes 8 (lr & 1) .. +7 of token lc
            const uint2 raw = *reinterpret_cast<const uint2*>(
                sbuf + b * kBlkBytes + ((2 * ds + (lr >> 1)) * 16 + lc) * 16 + 8 * (lr & 1));
            const uint2 lo = MfmaQK<T>::template from_fp8x4<E5M2>(raw.x);
            const uint2 hi = MfmaQK<T>::template from_fp8x4<E5M2>(raw.y);
            kf = make_uint4(lo.x, lo.y, hi.x, hi.y);
          }
#pragma unroll
          for (int qt = 0; qt < QT; ++qt) s[b][qt] = MfmaQK<T>::run(kf, qf[qt][ds], s[b][qt]);
        }
      }
      // ---- online softmax per query column, once per stage (scores in raw units; scale and log2(e) folded into
      // one fma in front of v_exp_f32; masking only on stages that reach past the wave's all-visible limit) ----
      uint4 pfrag[QT][kNB / 2];
      const bool need_mask = OPTS || (t0 + kKeys - 1) > wave_limit_lo;
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        float v[kNV];
        [[maybe_unused]] unsigned vis = ~0u;   // OPTS: which of the lane's keys this row sees
        if constexpr (OPTS) {
          const int qpos = ctx + qrow[qt];
          const int limit = min(qpos, seq_len - 1);
          const int first = window > 0 ? qpos - window + 1 : 0;
          vis = 0u;
#pragma unroll
          for (int b = 0; b < kNB; ++b) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int key = t0 + 16 * b + 4 * lr + j;
              float sv = s[b][qt][j] * scale;
              if (softcap > 0.f) {
                // cap * tanh(sv / cap), tanh(x) = 1 - 2 / (e^(2x) + 1)
                const float e = __builtin_amdgcn_exp2f(sv * cap_inv2);
                sv = softcap * (1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f));
              }
              const bool ok = key <= limit && key >= first;
              vis |= ok ? (1u << (b * 4 + j)) : 0u;
              v[b * 4 + j] = ok ? sv : kNegBig;
            }
          }
        } else if (need_mask) {
          const int limit = min(ctx + qrow[qt], seq_len - 1);  // last visible key of this row
#pragma unroll
          for (int b = 0; b < kNB; ++b) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int key = t0 + 16 * b + 4 * lr + j;
              v[b * 4 + j] = key <= limit ? s[b][qt][j] : kNegBig;   // (also drops NaN of dead keys)
            }
          }
        } else {
#pragma unroll
          for (int b = 0; b < kNB; ++b) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[b * 4 + j] = s[b][qt][j];
          }
        }
        float tmax = v[0];
#pragma unroll
        for (int i = 1; i < kNV; ++i) tmax = fmaxf(tmax, v[i]);
        tmax = rows_max(tmax);
        const float mnew = fmaxf(mrun[qt], tmax);
        const float alpha = __builtin_amdgcn_exp2f((mrun[qt] - mnew) * sl2);
        mrun[qt] = mnew;
        const float mc = -mnew * sl2;
        float psum = 0.f;
#pragma unroll
        for (int i = 0; i < kNV; ++i) {
          v[i] = __builtin_amdgcn_exp2f(fmaf(v[i], sl2, mc));
          // OPTS: a row whose window has not started yet has NO visible key in this stage: its running maximum is
          // still the sentinel and 2^(sentinel - sentinel) would count every masked key as 1
          if constexpr (OPTS) v[i] = (vis >> i) & 1u ? v[i] : 0.f;
          psum += v[i];
        }
        lrun[qt] = lrun[qt] * alpha + psum;
        if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {
#pragma unroll
          for (int dt = 0; dt < kDT; ++dt) {
            oacc[qt][dt][0] *= alpha;
            oacc[qt][dt][1] *= alpha;
            oacc[qt][dt][2] *= alpha;
            oacc[qt][dt][3] *= alpha;
          }
        }
        // PV step h takes blocks 2h (k index 8 lr + 0..3) and 2h + 1 (8 lr + 4..7)
#pragma unroll
        for (int h = 0; h < kNB / 2; ++h) {
          pfrag[qt][h].x = MfmaQK<T>::pack(v[8 * h + 0], v[8 * h + 1]);
          pfrag[qt][h].y = MfmaQK<T>::pack(v[8 * h + 2], v[8 * h + 3]);
          pfrag[qt][h].z = MfmaQK<T>::pack(v[8 * h + 4], v[8 * h + 5]);
          pfrag[qt][h].w = MfmaQK<T>::pack(v[8 * h + 6], v[8 * h + 7]);
        }
      }
      // ---- O^T += V^T . P^T: 32 keys per step ------------------------------------------------
      const char* vimg = sbuf + kNB * kBlkBytes;
#pragma unroll
      for (int h = 0; h < kNB / 2; ++h) {
#pragma unroll
        for (int dt = 0; dt < kDT; ++dt) {
          // V block image [HD d][16 keys]: row 16*dt + lc, keys 4*lr .. 4*lr+3 (8 bytes; 4 for fp8)
          uint2 v0, v1;
          if constexpr (!KV8) {
            v0 = *reinterpret_cast<const uint2*>(vimg + (2 * h) * kBlkBytes + (16 * dt + lc) * 32 + 8 * lr);
            v1 = *reinterpret_cast<const uint2*>(vimg + (2 * h + 1) * kBlkBytes + (16 * dt + lc) * 32 + 8 * lr);
          } else {
            v0 = MfmaQK<T>::template from_fp8x4<E5M2>(*reinterpret_cast<const uint32_t*>(
                vimg + (2 * h) * kBlkBytes + (16 * dt + lc) * 16 + 4 * lr));
            v1 = MfmaQK<T>::template from_fp8x4<E5M2>(*reinterpret_cast<const uint32_t*>(
                vimg + (2 * h + 1) * kBlkBytes + (16 * dt + lc) * 16 + 4 * lr));
          }
          const uint4 vf = make_uint4(v0.x, v0.y, v1.x, v1.y);
#pragma unroll
          for (int qt = 0; qt < QT; ++qt) oacc[qt][dt] = MfmaQK<T>::run(vf, pfrag[qt][h], oacc[qt][dt]);
        }
      }
    }
    cur = cur + 1 == kHdStages ? 0 : cur + 1;
  }

  // ---- epilogue: O[q][d] = O^T[d][q] / l ----------------------------------------------
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    float inv = 1.0f / rows_sum(lrun[qt]);
    if constexpr (KV8) inv *= *v_scale;
    if (qrow[qt] < q_len) {
      T* op = out + (int64_t)(q_begin + qrow[qt]) * out_stride + (int64_t)head * HD + 4 * lr;
#pragma unroll
      for (int dt = 0; dt < kDT; ++dt) {
        const uint2 v = make_uint2(MfmaQK<T>::pack(oacc[qt][dt][0] * inv, oacc[qt][dt][1] * inv),
                                   MfmaQK<T>::pack(oacc[qt][dt][2] * inv, oacc[qt][dt][3] * inv));
        *reinterpret_cast<uint2*>(op + 16 * dt) = v;
      }
    }
  }
}

// one instantiation: reserve its LDS ring once per device where it exceeds the 64 KiB a kernel gets by default
// (HD 256 with a 16-bit cache: 96 KiB), then launch
template <typename T, int HD, bool KV8, bool OPTS, bool E5M2, int QT, int NW>
static int hd_launch_v(const PrefillArgs& a) {
  constexpr int kSmem = HdShape<HD, KV8>::kSmem;
  auto kern = paged_prefill_hd_kernel<T, HD, KV8, OPTS, E5M2, QT, NW>;
  if constexpr (kSmem > 64 * 1024) {
    static PerDeviceOnce once;   // one per instantiation, one bit per device
    int dev;
    if (once.need(&dev)) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, kSmem);
      if (e != hipSuccess) {
        set_error("paged_prefill_attention(hd): cannot reserve %d B of LDS: %s", kSmem, hipGetErrorString(e));
        return MI355X_EUNSUPPORTED;
      }
      once.mark(dev);
    }
  }
  const int q_blocks = (a.max_query_len + 16 * NW * QT - 1) / (16 * NW * QT);
  hipLaunchKernelGGL(kern, dim3(a.num_seqs * q_blocks * a.num_heads), dim3(64 * NW), kSmem, a.stream,
                     static_cast<T*>(a.out), static_cast<const T*>(a.query), a.key_cache, a.value_cache,
                     a.num_heads, a.num_kv_heads, a.scale, a.block_tables, a.seq_lens, a.cu_seqlens_q,
                     a.max_num_blocks_per_seq, q_blocks, a.q_stride, a.out_stride, a.kv_block_stride,
                     a.kv_head_stride, a.k_scale, a.v_scale, OPTS ? a.sliding_window : 0, OPTS ? a.softcap : 0.f);
  return check_launch(OPTS ? "paged_prefill_attention(hd, opts)" : "paged_prefill_attention(hd)");
}

// the workgroup shape (QT tiles per wave, NW waves) of one (T, HD, KV8, OPTS, E5M2) combination
template <typename T, int HD, bool KV8, bool OPTS, bool E5M2>
static int hd_launch_one(const PrefillArgs& a) {
  static_assert(HdShape<HD, KV8>::kSmem <= 160 * 1024, "LDS of one CU");
  if constexpr (HD == 256) {
    return hd_launch_v<T, HD, KV8, OPTS, E5M2, 1, 8>(a);
  } else {
    // 128 query rows per workgroup — 64 when that makes fewer than 512 workgroups (the rule of the d128 launcher)
    const int64_t wgs128 = (int64_t)a.num_seqs * ((a.max_query_len + 127) / 128) * a.num_heads;
    return wgs128 < 512 ? hd_launch_v<T, HD, KV8, OPTS, E5M2, 1, 4>(a) : hd_launch_v<T, HD, KV8, OPTS, E5M2, 2, 4>(a);
  }
}

template <typename T, int HD>
static int hd_launch_t(const PrefillArgs& a) {
  const bool kv8 = a.kv_cache_dtype != MI355X_KV_AUTO;
  const bool e5m2 = a.kv_cache_dtype == MI355X_KV_FP8_E5M2;
  if (a.sliding_window > 0 || a.softcap > 0.f) {
    if (kv8 && e5m2) return hd_launch_one<T, HD, true, true, true>(a);
    if (kv8) return hd_launch_one<T, HD, true, true, false>(a);
    return hd_launch_one<T, HD, false, true, false>(a);
  }
  if (kv8 && e5m2) return hd_launch_one<T, HD, true, false, true>(a);
  if (kv8) return hd_launch_one<T, HD, true, false, false>(a);
  return hd_launch_one<T, HD, false, false, false>(a);
}

int paged_prefill_hd_launch(const PrefillArgs& a) {
  return MI355X_DISPATCH_HALF(a.dtype, [&] {
    return a.head_size == 64 ? hd_launch_t<scalar_t, 64>(a) : hd_launch_t<scalar_t, 256>(a);
  });
}

}  // namespace mi355x
