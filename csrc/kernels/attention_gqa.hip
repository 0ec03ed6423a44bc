// Grouped-query flash attention for gfx950: the GQA siblings of the
// kernels in attention.hip, on the same tile bodies (attn_tiles.h).  A
// translation unit of its own, so that the MHA instantiations compile to
// the code they compiled to before these kernels existed.

#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

#include "attn_tiles.h"

namespace {

// ============================================================================
// Grouped-query attention (GQA): H query heads, Hkv = H / G kv heads, query
// head h reads kv head h / G (the repeat_interleave order).  Sibling
// kernels of the four split kernels of attention.hip — bf16, d64 / d128,
// causal or not, seqlens; no dropout, no dlse — on the same tile bodies,
// so the MHA instantiations keep their arguments and their registers.  K and V are [B, Hkv, S, D]
// with strides of their own (kv_s*), dK and dV likewise (g_s* of the
// kv-parallel kernel); q, out, dO, dQ, lse and delta stay per query head.
//
// The kernels of this file (and the tile bodies inlined into them) are
// compiled with the packed fp32 instructions (v_pk_mul_f32 and kin) turned
// off: a choice of instruction selection for new kernels, not of
// arithmetic — the scalar forms compute the same fp32 values.  Registers
// with and without it are in docs/kernels.md; the MHA kernels keep the
// selection they were measured and validated with.
// ============================================================================
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                   \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// q-parallel GQA grids: non-causal dim3(n * G, B * Hkv), causal
// dim3(B * H, n); both in the group-aware order of attn_block_order.h.
// A build with -DEPL_ATTN_GQA_PLAIN_ORDER keeps bh = blockIdx.x on the
// causal grid: the other side of the A/B in tests/attn_gqa_perf_gpu.py.
DEVI BlockPos block_pos_gqa(int causal, unsigned int group) {
  if (causal) {
#ifdef EPL_ATTN_GQA_PLAIN_ORDER
    const unsigned int bh = blockIdx.x;
#else
    const unsigned int bh = attn_order::causal_group_bh(blockIdx.x, group,
                                                        gridDim.x / group);
#endif
    return {(int64_t)bh, (int64_t)gridDim.y - 1 - blockIdx.y};
  }
  const attn_order::Block b = attn_order::block_of_group(
      blockIdx.x, blockIdx.y, gridDim.x / group, group, gridDim.y);
  return {(int64_t)b.bh, (int64_t)b.blk};
}

// forward: attn_fwd_kernel<false, D> (attention.hip) with kv-side strides
// and the group-aware block position.  The two are twins: a fix to the
// loop structure, the staging or the epilogue of one belongs in the other.
template <int D>
__global__ __launch_bounds__(256, D == 64 ? 3 : 2) void attn_fwd_gqa_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, short* __restrict__ out,
    float* __restrict__ lse, int64_t seq, float scale, int causal,
    int64_t heads, int64_t group, int64_t in_sb, int64_t in_sh,
    int64_t in_ss, int64_t kv_sb, int64_t kv_sh, int64_t kv_ss,
    int64_t o_sb, int64_t o_sh, int64_t o_ss,
    const int* __restrict__ seqlens) {
  __shared__ __attribute__((aligned(16))) short
      ldsV[2][64 * img_pitch<D>()];
  __shared__ __attribute__((aligned(16))) short ldsK[2][64][D + 8];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int hi = lane >> 5;
  const int lq = lane & 31;
  const BlockPos pos = block_pos_gqa(causal, (unsigned int)group);
  const int64_t bh = pos.bh;
  const int64_t b = bh / heads, h = bh % heads;
  const int64_t q0_blk = pos.blk * 128;
  const int64_t q0 = q0_blk + wave * 32;
  const int64_t len = sample_len(seqlens, b, seq);
  const int64_t myq = q0 + lq;
  short* ob = out + b * o_sb + h * o_sh;
  if (myq >= len && myq < seq) {
    zero_row<D>(ob + myq * o_ss, hi);
    if (hi == 0) lse[bh * seq + myq] = 0.f;
  }
  if (q0_blk >= len) return;
  const bool active = q0 < len;
  const short* qp = q + b * in_sb + h * in_sh;
  const int64_t kvoff = b * kv_sb + (h / group) * kv_sh;
  const short* kp = k + kvoff;
  const short* vp = v + kvoff;

  const int64_t qrow = myq < len ? myq : len - 1;
  bf16x8 qfrag[D / 16];
#pragma unroll
  for (int c = 0; c < D / 16; ++c)
    qfrag[c] = *reinterpret_cast<const bf16x8*>(
        qp + qrow * in_ss + hi * 8 + 16 * c);

  f32x16 ot[D / 32] = {};
  float m = -1e30f, l = 0.f;
  const float c2 = scale * 1.44269504088896341f;
  const int64_t len64 = len & ~(int64_t)63;
  const int64_t bulk_end = causal ? (q0_blk < len64 ? q0_blk : len64) : len64;
  const int64_t blk_kv_end =
      causal ? (q0_blk + 128 < len ? q0_blk + 128 : len) : len;

  // the MHA forward's single-barrier double-buffered staging
  const int stage_row = threadIdx.x >> 3;
  const int stage_seg = (threadIdx.x & 7) * 8;
  bf16x8 pv[2][D / 64], pk[2][D / 64];
  auto load_tile = [&](int64_t kv0) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      int64_t vrow = kv0 + stage_row + half * 32;
      if (vrow >= len) vrow = len - 1;
#pragma unroll
      for (int s = 0; s < D / 64; ++s) {
        const int col = stage_seg + s * 64;
        pv[half][s] =
            *reinterpret_cast<const bf16x8*>(vp + vrow * kv_ss + col);
        pk[half][s] =
            *reinterpret_cast<const bf16x8*>(kp + vrow * kv_ss + col);
      }
    }
  };
  auto write_tile = [&](int buf) {
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int s = 0; s < D / 64; ++s) {
        const int row = stage_row + half * 32;
        const int col = stage_seg + s * 64;
        *reinterpret_cast<bf16x8*>(
            &ldsV[buf][img_off<D>(row, col >> 3)]) = pv[half][s];
        *reinterpret_cast<bf16x8*>(&ldsK[buf][row][col]) = pk[half][s];
      }
  };
  auto tile = [&](auto masked, int buf, int sub, int64_t kvs) {
    constexpr bool M = decltype(masked)::value;
    fwd_tile<M, false, D>(ldsK[buf], ldsV[buf], sub, kvs, len, myq, c2,
                          causal, qfrag, ot, m, l, lq, hi, nullptr, 0, 0u,
                          0u, 0u, 0, 1.f);
  };
  constexpr std::true_type MASKED_T{};
  constexpr std::false_type PLAIN_T{};

  int buf = 0;
  if (blk_kv_end > 0) load_tile(0);
  int64_t kv0 = 0;
  for (; kv0 < bulk_end; kv0 += 64) {
    write_tile(buf);
    __syncthreads();
    if (kv0 + 64 < blk_kv_end) load_tile(kv0 + 64);
#pragma unroll
    for (int sub = 0; sub < 64; sub += 32)
      tile(PLAIN_T, buf, sub, kv0 + sub);
    buf ^= 1;
  }
  for (; kv0 < blk_kv_end; kv0 += 64) {
    write_tile(buf);
    __syncthreads();
    if (kv0 + 64 < blk_kv_end) load_tile(kv0 + 64);
    if (active) {
      const int64_t wave_kv_end = causal
          ? (q0 + 32 < len ? q0 + 32 : len) : len;
#pragma unroll
      for (int sub = 0; sub < 64; sub += 32) {
        const int64_t kvs = kv0 + sub;
        if (kvs >= wave_kv_end) break;
        tile(MASKED_T, buf, sub, kvs);
      }
    }
    buf ^= 1;
  }

  {
    unsigned int a, c;
    both_halves(__builtin_bit_cast(unsigned int, l), a, c);
    l = __builtin_bit_cast(float, a) + __builtin_bit_cast(float, c);
  }
  const float inv_l = 1.f / l;
  // O leaves through the freed K buffers as whole rows (see
  // attn_fwd_kernel); every wave of the block reaches both barriers
  short* ldsO = &ldsK[0][0][0] + wave * 32 * (D + 8);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < D / 32; ++j)
    store_acc_bf16(ldsO + lq * (D + 8) + j * 32, ot[j] * inv_l, hi);
  __syncthreads();
  constexpr int LPR = D / 8;
#pragma unroll
  for (int r0 = 0; r0 < 32; r0 += 64 / LPR) {
    const int r = r0 + lane / LPR;
    const int col = (lane % LPR) * 8;
    const bf16x8 piece =
        *reinterpret_cast<const bf16x8*>(ldsO + r * (D + 8) + col);
    if (q0 + r < len)
      *reinterpret_cast<bf16x8*>(ob + (q0 + r) * o_ss + col) = piece;
  }
  if (hi == 0 && myq < len) lse[bh * seq + myq] = m * scale + __logf(l);
}

// ----------------------------------------------------------------------------
// kv-parallel GQA backward: dV (DK = false) or dK (DK = true) of one
// batch-kv-head's 128 keys per block, SUMMED over the group's G query
// heads in registers.  A wave loads its 32 keys' K (and V) fragments once
// and keeps one set of fp32 accumulators; for g = 0 .. G-1 in ascending
// order it streams query head kvh * G + g's Q, dO, -lse/scale (and
// -delta) chunks through the LDS image and the split kernels' tile
// bodies.  Each output row is rounded to bf16 once and has one writer: no
// atomics, no workspace, a fixed summation order.
//
//  * q-side pointers and the lse / delta rows use the query head
//    b * H + kvh * G + g; the output row and sample_len use (b, kvh).
//    len depends on b alone, so every test on it stays block-uniform.
//  * the zero-fill of padded key rows and the early return happen once.
//  * DBUF = false (d128, causal): the direct two-barrier staging; the
//    causal phase split restarts for each g with the same bounds.
//  * DBUF = true (d64 non-causal dV only): register-double-buffered
//    single-barrier staging over the FLATTENED sequence of (g, chunk):
//    the chunk after the last chunk of head g is the first chunk of head
//    g + 1, so the pipeline fills once per block, not once per head.
// ----------------------------------------------------------------------------
template <bool DK, bool DBUF, int D>
__global__ __launch_bounds__(256, DK ? (D == 64 ? 3 : 2)
                                     : (D == 64 ? (DBUF ? 3 : 4) : 3))
void attn_bwd_kv_gqa_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, const short* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    short* __restrict__ dkv, int64_t seq, float scale, int causal,
    int64_t heads, int64_t group, int64_t in_sb, int64_t in_sh,
    int64_t in_ss, int64_t kv_sb, int64_t kv_sh, int64_t kv_ss,
    int64_t do_sb, int64_t do_sh, int64_t do_ss, int64_t g_sb,
    int64_t g_sh, int64_t g_ss, const int* __restrict__ seqlens) {
  constexpr int PITCH = img_pitch<D>();
  constexpr int NB = DBUF ? 2 : 1;
  constexpr int NC = DK ? 2 : 1;   // row constants: -lse/scale (, -delta)
  __shared__ __attribute__((aligned(16))) short ldsQ[NB][64][PITCH];
  __shared__ __attribute__((aligned(16))) short ldsDO[NB][64][PITCH];
  __shared__ __attribute__((aligned(16))) float ldsL[NB][NC][64];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int hi = lane >> 5;
  const int lkv = lane & 31;
  // plain block_pos over the B * Hkv batch-kv-heads: the axes and the
  // order of the MHA dV / dK grids
  const BlockPos pos = block_pos(causal, false);
  const int64_t kv_heads = heads / group;
  const int64_t b = pos.bh / kv_heads, kvh = pos.bh % kv_heads;
  const int64_t kv0_blk = pos.blk * 128;
  const int64_t kv0 = kv0_blk + wave * 32;
  const int64_t len = sample_len(seqlens, b, seq);
  const int64_t mykv = kv0 + lkv;
  const int64_t goff = b * g_sb + kvh * g_sh + mykv * g_ss;
  if (mykv >= len && mykv < seq) zero_row<D>(dkv + goff, hi);
  if (kv0_blk >= len) return;
  const bool active = kv0 < len;

  const int64_t kvrow = mykv < len ? mykv : len - 1;
  const int64_t kvoff = b * kv_sb + kvh * kv_sh + kvrow * kv_ss + hi * 8;
  bf16x8 kfrag[D / 16], vfrag[D / 16];
#pragma unroll
  for (int c = 0; c < D / 16; ++c) {
    kfrag[c] = *reinterpret_cast<const bf16x8*>(k + kvoff + 16 * c);
    if (DK) vfrag[c] = *reinterpret_cast<const bf16x8*>(v + kvoff + 16 * c);
  }

  // the group's first query head; head g sits g * in_sh (do_sh, seq)
  // further
  const int64_t h0 = kvh * group;
  const short* qg = q + b * in_sb + h0 * in_sh;
  const short* dog = dout + b * do_sb + h0 * do_sh;
  const float* lseg = lse + (b * heads + h0) * seq;
  const float* dltg = DK ? delta + (b * heads + h0) * seq : nullptr;

  f32x16 acc[D / 32] = {};
  const int stage_row = threadIdx.x >> 3;
  const int stage_seg = (threadIdx.x & 7) * 8;
  const float neg_inv_scale = -1.f / scale;
  // wave 0 carries the chunk's -lse/scale values, wave 1 (dK) -delta
  auto row_const = [&](int64_t g, int64_t q0) {
    const int64_t qr = q0 + lane;
    const float* p = (wave == 0 ? lseg : dltg) + g * seq;
    return p[qr < len ? qr : len - 1] * (wave == 0 ? neg_inv_scale : -1.f);
  };
  bf16x8 rq[2][D / 64], rdo[2][D / 64];
  float rl = 0.f;
  auto prefetch = [&](int64_t g, int64_t q0) {
    if (wave < NC) rl = row_const(g, q0);
    const short* qp = qg + g * in_sh;
    const short* dop = dog + g * do_sh;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      int64_t qr = q0 + stage_row + half * 32;
      if (qr >= len) qr = len - 1;
#pragma unroll
      for (int s = 0; s < D / 64; ++s) {
        rq[half][s] = *reinterpret_cast<const bf16x8*>(
            qp + qr * in_ss + stage_seg + s * 64);
        rdo[half][s] = *reinterpret_cast<const bf16x8*>(
            dop + qr * do_ss + stage_seg + s * 64);
      }
    }
  };
  auto commit = [&](int buf) {
    if (wave < NC) ldsL[buf][wave][lane] = rl;
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int s = 0; s < D / 64; ++s) {
        *reinterpret_cast<bf16x8*>(
            img_at<D>(ldsQ[buf], stage_row + half * 32,
                      stage_seg + s * 64)) = rq[half][s];
        *reinterpret_cast<bf16x8*>(
            img_at<D>(ldsDO[buf], stage_row + half * 32,
                      stage_seg + s * 64)) = rdo[half][s];
      }
  };
  auto stage_q64 = [&](int64_t g, int64_t q0) {
    __syncthreads();
    prefetch(g, q0);
    commit(0);
    __syncthreads();
  };

  auto tile = [&](auto masked, int rb, int sub, int64_t q0s) {
    constexpr bool M = decltype(masked)::value;
    if constexpr (DK)
      dk_tile_tr<M, false, D>(&ldsQ[rb][0][0], &ldsDO[rb][0][0],
                              &ldsL[rb][0][sub], &ldsL[rb][1][sub], sub,
                              q0s, len, mykv, scale, causal, kfrag, vfrag,
                              acc, lkv, hi, nullptr, 0, 1.f);
    else
      dv_tile_tr<M, false, D>(&ldsQ[rb][0][0], &ldsDO[rb][0][0],
                              &ldsL[rb][0][sub], sub, q0s, len, mykv,
                              scale, causal, kfrag, acc, lkv, hi, nullptr,
                              0, 1.f);
  };
  constexpr std::true_type MASKED_T{};
  constexpr std::false_type PLAIN_T{};

  const int64_t bulk_end = len & ~(int64_t)63;
  if (!DBUF) {
    const int64_t diag_end =
        causal ? (kv0_blk + 128 < len ? kv0_blk + 128 : len) : 0;
    for (int64_t g = 0; g < group; ++g) {
      int64_t q0 = causal ? kv0_blk : 0;
      for (; q0 < diag_end; q0 += 64) {
        stage_q64(g, q0);
        if (!active) continue;
#pragma unroll
        for (int sub = 0; sub < 64; sub += 32) {
          const int64_t q0s = q0 + sub;
          if (q0s >= diag_end || (causal && q0s + 31 < kv0)) continue;
          tile(MASKED_T, 0, sub, q0s);
        }
      }
      q0 = diag_end > q0 ? diag_end : q0;
      for (; q0 + 63 < bulk_end; q0 += 64) {
        stage_q64(g, q0);
#pragma unroll
        for (int sub = 0; sub < 64; sub += 32)
          tile(PLAIN_T, 0, sub, q0 + sub);
      }
      for (; q0 < len; q0 += 64) {
        stage_q64(g, q0);
        if (!active) continue;
#pragma unroll
        for (int sub = 0; sub < 64; sub += 32) {
          const int64_t q0s = q0 + sub;
          if (q0s >= len) break;
          tile(MASKED_T, 0, sub, q0s);
        }
      }
    }
  } else {
    // non-causal: every head's chunks are q0 = 0, 64, .. < len (len > 0
    // here).  (g, q0) is the chunk in LDS buffer `buf` after the barrier,
    // (ng, nq0) the one in flight.
    int buf = 0;
    int64_t g = 0, q0 = 0;
    prefetch(0, 0);
    for (;;) {
      commit(buf);
      __syncthreads();
      int64_t ng = g, nq0 = q0 + 64;
      if (nq0 >= len) {
        ng = g + 1;
        nq0 = 0;
      }
      if (ng < group) prefetch(ng, nq0);
      const int rb = buf;
      buf ^= 1;
      if (q0 + 63 < bulk_end) {
#pragma unroll
        for (int sub = 0; sub < 64; sub += 32)
          tile(PLAIN_T, rb, sub, q0 + sub);
      } else if (active) {
#pragma unroll
        for (int sub = 0; sub < 64; sub += 32) {
          const int64_t q0s = q0 + sub;
          if (q0s >= len) break;
          tile(MASKED_T, rb, sub, q0s);
        }
      }
      if (ng >= group) break;
      g = ng;
      q0 = nq0;
    }
  }
  if (!active || mykv >= len) return;
#pragma unroll
  for (int dj = 0; dj < D / 32; ++dj)
    store_acc_bf16(dkv + goff + dj * 32, acc[dj], hi);
}

// dQ: attn_bwd_dq_kernel<false, D> (attention.hip) with kv-side strides
// and the group-aware block position — twins, like the forward: a fix to
// one belongs in the other.  Publishes delta per query head for the GQA
// dK kernel (launch order dV -> dQ -> dK)
template <int D>
__global__ __launch_bounds__(256, D == 64 ? 3 : 2) void attn_bwd_dq_gqa_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, const short* __restrict__ dout,
    const float* __restrict__ lse, float* __restrict__ delta,
    short* __restrict__ dq, const short* __restrict__ out, int64_t seq,
    float scale, int causal, int64_t heads, int64_t group, int64_t in_sb,
    int64_t in_sh, int64_t in_ss, int64_t kv_sb, int64_t kv_sh,
    int64_t kv_ss, int64_t do_sb, int64_t do_sh, int64_t do_ss,
    int64_t g_sb, int64_t g_sh, int64_t g_ss, int64_t o_sb, int64_t o_sh,
    int64_t o_ss, const int* __restrict__ seqlens) {
  __shared__ __attribute__((aligned(16))) short ldsK[64][img_pitch<D>()];
  __shared__ __attribute__((aligned(16))) short ldsVr[64][img_pitch<D>()];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int hi = lane >> 5;
  const int lq = lane & 31;
  const BlockPos pos = block_pos_gqa(causal, (unsigned int)group);
  const int64_t bh = pos.bh;
  const int64_t b = bh / heads, h = bh % heads;
  const int64_t q0_blk = pos.blk * 128;
  const int64_t q0 = q0_blk + wave * 32;
  const int64_t len = sample_len(seqlens, b, seq);
  const int64_t myq = q0 + lq;
  short* dqb = dq + b * g_sb + h * g_sh;
  if (myq >= len && myq < seq) zero_row<D>(dqb + myq * g_ss, hi);
  if (q0_blk >= len) return;
  const bool active = q0 < len;
  const short* qp = q + b * in_sb + h * in_sh;
  const int64_t kvoff = b * kv_sb + (h / group) * kv_sh;
  const short* kp = k + kvoff;
  const short* vp = v + kvoff;
  const short* dop = dout + b * do_sb + h * do_sh;
  const short* op_ = out + b * o_sb + h * o_sh;

  const int64_t qrow = myq < len ? myq : len - 1;
  const float mylse = lse[bh * seq + qrow];
  bf16x8 qfrag[D / 16], dofrag[D / 16];
  float dsum = 0.f;
#pragma unroll
  for (int c = 0; c < D / 16; ++c) {
    qfrag[c] = *reinterpret_cast<const bf16x8*>(
        qp + qrow * in_ss + hi * 8 + 16 * c);
    dofrag[c] = *reinterpret_cast<const bf16x8*>(
        dop + qrow * do_ss + hi * 8 + 16 * c);
    bf16x8 of = *reinterpret_cast<const bf16x8*>(
        op_ + qrow * o_ss + hi * 8 + 16 * c);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      dsum += bf2f(dofrag[c][j]) * bf2f(of[j]);
  }
  const float mydelta = dsum + __shfl_xor(dsum, 32, 64);
  if (myq < len && hi == 0) delta[bh * seq + myq] = mydelta;

  f32x16 dqt[D / 32] = {};
  const int stage_row = threadIdx.x >> 3;
  const int stage_seg = (threadIdx.x & 7) * 8;
  const int64_t len64 = len & ~(int64_t)63;
  const int64_t bulk_end = causal ? (q0_blk < len64 ? q0_blk : len64) : len64;
  const int64_t blk_kv_end =
      causal ? (q0_blk + 128 < len ? q0_blk + 128 : len) : len;

  auto stage_kv64 = [&](int64_t kv0) {
    __syncthreads();
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      int64_t kr = kv0 + stage_row + half * 32;
      if (kr >= len) kr = len - 1;   // dS there is 0
#pragma unroll
      for (int seg = 0; seg < D; seg += 64) {
        *reinterpret_cast<bf16x8*>(
            img_at<D>(ldsK, stage_row + half * 32, stage_seg + seg)) =
            *reinterpret_cast<const bf16x8*>(
                kp + kr * kv_ss + stage_seg + seg);
        *reinterpret_cast<bf16x8*>(
            img_at<D>(ldsVr, stage_row + half * 32, stage_seg + seg)) =
            *reinterpret_cast<const bf16x8*>(
                vp + kr * kv_ss + stage_seg + seg);
      }
    }
    __syncthreads();
  };
  auto tile = [&](auto masked, int sub, int64_t kvs) {
    constexpr bool M = decltype(masked)::value;
    dq_tile_tr<M, false, D>(&ldsK[0][0], &ldsVr[0][0], sub, kvs, len, myq,
                            scale, causal, mylse, mydelta, qfrag, dofrag,
                            dqt, lq, hi, nullptr, 0, 1.f);
  };
  constexpr std::true_type MASKED_T{};
  constexpr std::false_type PLAIN_T{};
  int64_t kv0 = 0;
  for (; kv0 < bulk_end; kv0 += 64) {
    stage_kv64(kv0);
#pragma unroll
    for (int sub = 0; sub < 64; sub += 32)
      tile(PLAIN_T, sub, kv0 + sub);
  }
  for (; kv0 < blk_kv_end; kv0 += 64) {
    stage_kv64(kv0);
    const int64_t wave_kv_end = causal
        ? (q0 + 32 < len ? q0 + 32 : len) : len;
    if (!active) continue;
#pragma unroll
    for (int sub = 0; sub < 64; sub += 32) {
      const int64_t kvs = kv0 + sub;
      if (kvs >= wave_kv_end) break;
      tile(MASKED_T, sub, kvs);
    }
  }

  if (!active || myq >= len) return;
#pragma unroll
  for (int dj = 0; dj < D / 32; ++dj)
    store_acc_bf16(dqb + myq * g_ss + dj * 32, dqt[dj], hi);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

}  // namespace

extern "C" {

void epl_attn_fwd_gqa(const void* q, const void* k, const void* v,
                      void* out, float* lse, int64_t batch_heads,
                      int64_t seq, float scale, bool causal, int64_t heads,
                      int64_t kv_heads, int64_t head_dim,
                      const int64_t* in_strides, const int64_t* kv_strides,
                      const int64_t* o_strides, const int* seqlens,
                      hipStream_t stream) {
  // GQA (no dropout: the binding refuses a mask): the q-parallel grids
  // of attn_block_order.h, dim3(n * G, B * Hkv) or causal dim3(B * H, n)
  const int64_t group = heads / kv_heads;
  const unsigned n = (unsigned)((seq + 127) / 128);
  const dim3 ggrid =
      causal ? dim3((unsigned)batch_heads, n)
             : dim3(n * (unsigned)group, (unsigned)(batch_heads / group));
#define FWD_GQA_ARGS                                                     \
  reinterpret_cast<const short*>(q), reinterpret_cast<const short*>(k),  \
    reinterpret_cast<const short*>(v), reinterpret_cast<short*>(out),  \
    lse, seq, scale, causal ? 1 : 0, heads, group, in_strides[0],      \
    in_strides[1], in_strides[2], kv_strides[0], kv_strides[1],        \
    kv_strides[2], o_strides[0], o_strides[1], o_strides[2], seqlens
  if (head_dim == 128)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(attn_fwd_gqa_kernel<128>), ggrid,
                       dim3(256), 0, stream, FWD_GQA_ARGS);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(attn_fwd_gqa_kernel<64>), ggrid,
                       dim3(256), 0, stream, FWD_GQA_ARGS);
#undef FWD_GQA_ARGS
}

void epl_attn_bwd_gqa(const void* q, const void* k, const void* v,
                      const void* out, const void* dout, const float* lse,
                      float* delta_ws, void* dq, void* dk, void* dv,
                      int64_t batch_heads, int64_t seq, float scale,
                      bool causal, int64_t heads, int64_t kv_heads,
                      int64_t head_dim, const int64_t* in_strides,
                      const int64_t* kv_strides, const int64_t* o_strides,
                      const int64_t* do_strides, const int64_t* g_strides,
                      const int64_t* gkv_strides, const int* seqlens,
                      hipStream_t stream) {
  // GQA (no dropout, no dlse: the binding refuses them), always the
  // split kernels: dV over the B * Hkv grid -> dQ over the group-aware
  // B * H grid (publishes delta per query head) -> dK.  d64 non-causal
  // runs the pipelined dV kernel; dK, causal and d128 stage directly.
  const int64_t group = heads / kv_heads;
  const int64_t bhkv = batch_heads / group;
  const unsigned n = (unsigned)((seq + 127) / 128);
  const dim3 kvgrid = causal ? dim3((unsigned)bhkv, n)
                             : dim3(n, (unsigned)bhkv);
  const dim3 qgrid = causal
                         ? dim3((unsigned)batch_heads, n)
                         : dim3(n * (unsigned)group, (unsigned)bhkv);
#define KV_GQA_ARGS(res)                                                 \
  reinterpret_cast<const short*>(q), reinterpret_cast<const short*>(k),  \
    reinterpret_cast<const short*>(v),                                 \
    reinterpret_cast<const short*>(dout), lse, delta_ws,               \
    reinterpret_cast<short*>(res), seq, scale, causal ? 1 : 0, heads,  \
    group, in_strides[0], in_strides[1], in_strides[2], kv_strides[0], \
    kv_strides[1], kv_strides[2], do_strides[0], do_strides[1],        \
    do_strides[2], gkv_strides[0], gkv_strides[1], gkv_strides[2],     \
    seqlens
  auto launch_gqa = [&](auto d_c, auto dbuf_c) {
    constexpr int D = decltype(d_c)::value;
    constexpr bool DBUF = decltype(dbuf_c)::value;
    // dK stages directly everywhere: at d64 non-causal the pipelined
    // form spills inside its bulk chunk loop and measured 5 % slower
    // (docs/kernels.md).  -DEPL_ATTN_GQA_DK_PIPELINED builds that side of
    // the A/B in tests/attn_gqa_perf_gpu.py.
#ifdef EPL_ATTN_GQA_DK_PIPELINED
    constexpr bool DBUF_K = DBUF;
#else
    constexpr bool DBUF_K = false;
#endif
    hipLaunchKernelGGL(
        HIP_KERNEL_NAME(attn_bwd_kv_gqa_kernel<false, DBUF, D>), kvgrid,
        dim3(256), 0, stream, KV_GQA_ARGS(dv));
    hipLaunchKernelGGL(
        HIP_KERNEL_NAME(attn_bwd_dq_gqa_kernel<D>), qgrid, dim3(256), 0,
        stream, reinterpret_cast<const short*>(q),
        reinterpret_cast<const short*>(k),
        reinterpret_cast<const short*>(v),
        reinterpret_cast<const short*>(dout), lse, delta_ws,
        reinterpret_cast<short*>(dq), reinterpret_cast<const short*>(out),
        seq, scale, causal ? 1 : 0, heads, group, in_strides[0],
        in_strides[1], in_strides[2], kv_strides[0], kv_strides[1],
        kv_strides[2], do_strides[0], do_strides[1], do_strides[2],
        g_strides[0], g_strides[1], g_strides[2], o_strides[0],
        o_strides[1], o_strides[2], seqlens);
    hipLaunchKernelGGL(
        HIP_KERNEL_NAME(attn_bwd_kv_gqa_kernel<true, DBUF_K, D>), kvgrid,
        dim3(256), 0, stream, KV_GQA_ARGS(dk));
  };
  using d64 = std::integral_constant<int, 64>;
  using d128 = std::integral_constant<int, 128>;
  if (head_dim == 128)
    launch_gqa(d128{}, std::false_type{});
  else if (causal)
    launch_gqa(d64{}, std::false_type{});
  else
    launch_gqa(d64{}, std::true_type{});
#undef KV_GQA_ARGS
}

}  // extern "C"
