// Banded causal flash attention for gfx950: packed documents and sliding
// windows.  Under a causal mask every query row i sees one contiguous
// interval of keys [kv_lo[i], i] and every key j is seen by one contiguous
// interval of queries [j, q_hi[j]); both bounds are non-decreasing along
// the sequence (ops/attention.py: band_bounds).  Four kernels, bf16,
// d64 / d128, causal only, no dropout, no dlse, on the GQA signature
// (G = 1 is MHA) plus one int32 bound row per sample (bound_sb = 0: one
// row broadcast over the batch).  A translation unit of its own, so that
// the MHA and the GQA instantiations compile to the code they compiled to
// before these kernels existed; the bulk phases run the plain tile bodies
// of attn_tiles.h, the masked phases the banded copies below.
//
//  * loop bounds are block-uniform and come from one scalar read each:
//    the bounds are monotone, so the block's first row holds the minimum
//    kv_lo and its last key the maximum q_hi (readfirstlane, as
//    sample_len).
//  * three phases.  forward / dQ: masked HEAD tiles (partly hidden from
//    some row of the block), branch-free BULK tiles, the masked DIAGONAL.
//    dK / dV: the DIAGONAL chunks, BULK chunks, a masked TAIL.
//  * inside the masked phases a wave skips the 32-wide sub-tiles that its
//    first row (forward / dQ) or its last key (dK / dV) cannot see; the
//    tests are wave-uniform (tr_frag needs EXEC all ones).
//  * every bound is clamped where it is read: kv_lo to [0, i], q_hi to
//    [j + 1, len].  Values that break monotonicity give a wrong visible
//    set, never an access outside the sample's rows, and every valid row
//    keeps its diagonal, so no softmax row is empty.
//
// With one document and window >= S every bound is trivial, the HEAD and
// TAIL phases do what the GQA kernels' masked phases do, and the results
// are the causal kernels' bits.

#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

#include "attn_tiles.h"

namespace {

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                   \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// kv_lo of row i (0 <= i < len), clamped to [0, i]
DEVI int64_t lo_at(const int* kv_lo, int64_t i) {
  const int64_t x = kv_lo[i];
  return x < 0 ? 0 : (x > i ? i : x);
}

// q_hi of key j (0 <= j < len), clamped to [j + 1, len]
DEVI int64_t hi_at(const int* q_hi, int64_t j, int64_t len) {
  const int64_t x = q_hi[j];
  return x <= j ? j + 1 : (x > len ? len : x);
}

DEVI int64_t uniform(int64_t x) {
  return __builtin_amdgcn_readfirstlane((int)x);
}

// fwd_tile<true, false, D> (attn_tiles.h) with the interval mask
// kvg < mylo || kvg > myq || kvg >= len.  A hidden key's P is set to an
// exact 0 after the exponential.  The -1e30 score alone is not enough
// here: a row whose first visited sub-tiles hide every key still has
// m = -1e30, so exp2((s - m) * c2) = exp2(0) = 1 per hidden key would go
// into l and ot, and it would be wiped only if the row's first real key
// forced a rescale with alpha = 0 — which the deferred rescale
// (kRescaleThr) does not promise.  With P masked, l and ot of such a row
// stay exact zeros until its first visible key, whose score then exceeds
// m = -1e30 by more than the threshold and sets m; nothing depends on the
// wipe.  Where a row has already seen a key, exp2 of a -1e30 score is an
// exact 0 anyway, so the diagonal tiles compute what the causal kernels'
// compute.
template <int D>
DEVI void fwd_tile_band(const short (&ldsK)[64][D + 8], const short* imgV,
                        int sub, int64_t kvs, int64_t len, int64_t myq,
                        int mylo, float c2,
                        const bf16x8 (&qfrag)[D / 16], f32x16 (&ot)[D / 32],
                        float& m, float& l, int lq, int hi) {
  f32x16 st = {};
#pragma unroll
  for (int c = 0; c < D / 16; ++c) {
    bf16x8 kfrag =
        *reinterpret_cast<const bf16x8*>(&ldsK[sub + lq][hi * 8 + 16 * c]);
    st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfrag, qfrag[c], st, 0, 0,
                                                 0);
  }
  float s[16];
  unsigned int hidden = 0;
  float tile_max = -1e30f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float sv = st[r];
    const int64_t kvg = kvs + crow(r, hi);
    if (kvg < mylo || kvg > myq || kvg >= len) {
      sv = -1e30f;
      hidden |= 1u << r;
    }
    s[r] = sv;
    tile_max = fmaxf(tile_max, sv);
  }
  {
    unsigned int a, b;
    both_halves(__builtin_bit_cast(unsigned int, tile_max), a, b);
    tile_max = fmaxf(__builtin_bit_cast(float, a),
                     __builtin_bit_cast(float, b));
  }
  if (__builtin_amdgcn_ballot_w64((tile_max - m) * c2 > kRescaleThr) != 0) {
    const float m_new = fmaxf(m, tile_max);
    const float alpha = __builtin_amdgcn_exp2f((m - m_new) * c2);
    m = m_new;
    l *= alpha;
#pragma unroll
    for (int j = 0; j < D / 32; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        ot[j][r] *= alpha;
  }
  const float nmc = -m * c2;
  float rowsum = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], c2, nmc));
    s[r] = (hidden >> r) & 1u ? 0.f : p;
    rowsum += s[r];
  }
  l += rowsum;
  bf16x8 pf0 = assemble_pfrag(&s[0]);
  bf16x8 pf1 = assemble_pfrag(&s[8]);
#pragma unroll
  for (int kc = 0; kc < 2; ++kc) {
    bf16x8 pf = kc == 0 ? pf0 : pf1;
#pragma unroll
    for (int j = 0; j < D / 32; ++j) {
      bf16x8 vt = tr_frag<D>(imgV, sub + 16 * kc, j, hi * 32 + lq);
      ot[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vt, pf, ot[j], 0, 0,
                                                      0);
    }
  }
}

// dq_tile_tr<true, false, D> with the interval mask
template <int D>
DEVI void dq_tile_band(const short* imgK, const short* imgV, int sub,
                       int64_t kv0, int64_t len, int64_t myq, int mylo,
                       float scale, float mylse, float mydelta,
                       const bf16x8 (&qfrag)[D / 16],
                       const bf16x8 (&dofrag)[D / 16],
                       f32x16 (&dqt)[D / 32], int lq, int hi) {
  f32x16 st = {};
  f32x16 dpt = {};
#pragma unroll
  for (int c = 0; c < D / 16; ++c) {
    const int o = img_off<D>(sub + lq, 2 * c + hi);
    bf16x8 kf = *reinterpret_cast<const bf16x8*>(imgK + o);
    bf16x8 vf = *reinterpret_cast<const bf16x8*>(imgV + o);
    st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qfrag[c], st, 0, 0, 0);
    dpt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, dofrag[c], dpt, 0, 0,
                                                  0);
  }
  float ds[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float pv = __expf(st[r] * scale - mylse);
    const int64_t kvg = kv0 + crow(r, hi);
    if (myq >= len || kvg >= len || kvg > myq || kvg < mylo) pv = 0.f;
    ds[r] = pv * (dpt[r] - mydelta) * scale;
  }
  bf16x8 db0 = assemble_pfrag(&ds[0]);
  bf16x8 db1 = assemble_pfrag(&ds[8]);
  const int lane = hi * 32 + lq;
#pragma unroll
  for (int kc = 0; kc < 2; ++kc) {
    bf16x8 db = kc == 0 ? db0 : db1;
#pragma unroll
    for (int dj = 0; dj < D / 32; ++dj) {
      bf16x8 kt = tr_frag<D>(imgK, sub + kc * 16, dj, lane);
      dqt[dj] =
          __builtin_amdgcn_mfma_f32_32x32x16_bf16(kt, db, dqt[dj], 0, 0, 0);
    }
  }
}

// the causal RowMask of key mykv over the 32 query rows from q0, its
// upper bound shrunk to the key's q_hi: still two 32-bit compares
DEVI RowMask band_mask(int64_t q0, int64_t len, int64_t mykv, int myhi) {
  RowMask rm(q0, len, mykv, 1);
  const int64_t h = (int64_t)myhi - q0;
  if (h < rm.hi_) rm.hi_ = h < 0 ? 0 : (int)h;
  return rm;
}

// dv_tile_tr<true, false, D> with the band mask
template <int D>
DEVI void dv_tile_band(const short* imgQ, const short* imgDO,
                       const float* lseL, int sub, int64_t q0, int64_t len,
                       int64_t mykv, int myhi, float scale,
                       const bf16x8 (&kfrag)[D / 16], f32x16 (&dvt)[D / 32],
                       int lkv, int hi) {
  f32x16 st = load_rowconst(lseL, hi);
#pragma unroll
  for (int c = 0; c < D / 16; ++c) {
    bf16x8 qf = *reinterpret_cast<const bf16x8*>(
        imgQ + img_off<D>(sub + lkv, 2 * c + hi));
    st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf, kfrag[c], st, 0, 0, 0);
  }
  const float c2 = scale * 1.44269504088896341f;   // P = exp2(c2 * S')
  const RowMask rm = band_mask(q0, len, mykv, myhi);
  float p[16];
#pragma unroll
  for (int r = 0; r < 16; ++r)
    p[r] = rm.masked(crow(r, hi)) ? 0.f
                                  : __builtin_amdgcn_exp2f(st[r] * c2);
  bf16x8 pb0 = assemble_pfrag(&p[0]);
  bf16x8 pb1 = assemble_pfrag(&p[8]);
  const int lane = hi * 32 + lkv;
#pragma unroll
  for (int qc = 0; qc < 2; ++qc) {
    bf16x8 pb = qc == 0 ? pb0 : pb1;
#pragma unroll
    for (int dj = 0; dj < D / 32; ++dj) {
      bf16x8 dot = tr_frag<D>(imgDO, sub + qc * 16, dj, lane);
      dvt[dj] =
          __builtin_amdgcn_mfma_f32_32x32x16_bf16(dot, pb, dvt[dj], 0, 0, 0);
    }
  }
}

// dk_tile_tr<true, false, D> with the band mask
template <int D>
DEVI void dk_tile_band(const short* imgQ, const short* imgDO,
                       const float* lseL, const float* dltL, int sub,
                       int64_t q0, int64_t len, int64_t mykv, int myhi,
                       float scale, const bf16x8 (&kfrag)[D / 16],
                       const bf16x8 (&vfrag)[D / 16], f32x16 (&dkt)[D / 32],
                       int lkv, int hi) {
  f32x16 st = load_rowconst(lseL, hi);
  f32x16 dpt = load_rowconst(dltL, hi);
#pragma unroll
  for (int c = 0; c < D / 16; ++c) {
    const int o = img_off<D>(sub + lkv, 2 * c + hi);
    bf16x8 qf = *reinterpret_cast<const bf16x8*>(imgQ + o);
    bf16x8 dof = *reinterpret_cast<const bf16x8*>(imgDO + o);
    st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf, kfrag[c], st, 0, 0, 0);
    dpt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dof, vfrag[c], dpt, 0, 0,
                                                  0);
  }
  const float c2 = scale * 1.44269504088896341f;   // P = exp2(c2 * S')
  const RowMask rm = band_mask(q0, len, mykv, myhi);
  float ds[16];
#pragma unroll
  for (int r = 0; r < 16; ++r)
    ds[r] = rm.masked(crow(r, hi))
                ? 0.f
                : __builtin_amdgcn_exp2f(st[r] * c2) * dpt[r] * scale;
  bf16x8 db0 = assemble_pfrag(&ds[0]);
  bf16x8 db1 = assemble_pfrag(&ds[8]);
  const int lane = hi * 32 + lkv;
#pragma unroll
  for (int qc = 0; qc < 2; ++qc) {
    bf16x8 db = qc == 0 ? db0 : db1;
#pragma unroll
    for (int dj = 0; dj < D / 32; ++dj) {
      bf16x8 qt = tr_frag<D>(imgQ, sub + qc * 16, dj, lane);
      dkt[dj] =
          __builtin_amdgcn_mfma_f32_32x32x16_bf16(qt, db, dkt[dj], 0, 0, 0);
    }
  }
}

// the causal q-parallel grid dim3(B * H, n) in the group-aware order of
// attention_gqa.hip.  Longest-first assumes that work grows with the block
// index, which a band breaks; the order is left as it is (docs/kernels.md)
DEVI BlockPos block_pos_band(unsigned int group) {
  const unsigned int bh =
      attn_order::causal_group_bh(blockIdx.x, group, gridDim.x / group);
  return {(int64_t)bh, (int64_t)gridDim.y - 1 - blockIdx.y};
}

// the kv loop of a forward / dQ block of rows [q0_blk, q0_blk + 128),
// q0_blk < len: tiles of 64 keys from `begin`; masked up to `head_end`,
// plain up to `bulk_end`, masked up to `end`
struct KvPhases {
  int64_t begin, head_end, bulk_end, end;
};
DEVI KvPhases kv_phases(const int* lo_row, int64_t q0_blk, int64_t len) {
  const int64_t last = q0_blk + 127 < len ? q0_blk + 127 : len - 1;
  const int64_t len64 = len & ~(int64_t)63;
  KvPhases p;
  p.begin = uniform(lo_at(lo_row, q0_blk)) & ~(int64_t)63;
  p.end = q0_blk + 128 < len ? q0_blk + 128 : len;
  const int64_t head = (uniform(lo_at(lo_row, last)) + 63) & ~(int64_t)63;
  p.head_end = head < p.end ? head : p.end;
  p.bulk_end = q0_blk < len64 ? q0_blk : len64;
  return p;
}

// forward: attn_fwd_gqa_kernel's causal path — the single-barrier
// double-buffered staging, the LDS epilogue — with the kv loop starting
// at the block's first visible tile and a masked head phase before the
// bulk.  The first staged tile, the prefetch guard and the buffer parity
// all count from ph.begin.
template <int D>
__global__ __launch_bounds__(256, D == 64 ? 3 : 2) void attn_fwd_band_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, short* __restrict__ out,
    float* __restrict__ lse, int64_t seq, float scale, int64_t heads,
    int64_t group, int64_t in_sb, int64_t in_sh, int64_t in_ss,
    int64_t kv_sb, int64_t kv_sh, int64_t kv_ss, int64_t o_sb, int64_t o_sh,
    int64_t o_ss, const int* __restrict__ seqlens,
    const int* __restrict__ kv_lo, int64_t bound_sb) {
  __shared__ __attribute__((aligned(16))) short
      ldsV[2][64 * img_pitch<D>()];
  __shared__ __attribute__((aligned(16))) short ldsK[2][64][D + 8];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int hi = lane >> 5;
  const int lq = lane & 31;
  const BlockPos pos = block_pos_band((unsigned int)group);
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
  const int* lo_row = kv_lo + b * bound_sb;

  const int64_t qrow = myq < len ? myq : len - 1;
  const int mylo = (int)lo_at(lo_row, qrow);
  // the wave's first row holds the minimum of its rows' bounds
  const int64_t wave_lo = uniform(lo_at(lo_row, active ? q0 : len - 1));
  bf16x8 qfrag[D / 16];
#pragma unroll
  for (int c = 0; c < D / 16; ++c)
    qfrag[c] = *reinterpret_cast<const bf16x8*>(
        qp + qrow * in_ss + hi * 8 + 16 * c);

  f32x16 ot[D / 32] = {};
  float m = -1e30f, l = 0.f;
  const float c2 = scale * 1.44269504088896341f;
  const KvPhases ph = kv_phases(lo_row, q0_blk, len);

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
  const int64_t wave_kv_end = q0 + 32 < len ? q0 + 32 : len;
  // one masked 64-key tile: the wave's sub-tiles between its first row's
  // lower bound and its diagonal
  auto masked_tile = [&](int buf, int64_t kv0) {
    if (!active) return;
#pragma unroll
    for (int sub = 0; sub < 64; sub += 32) {
      const int64_t kvs = kv0 + sub;
      if (kvs >= wave_kv_end) break;
      if (kvs + 32 <= wave_lo) continue;
      fwd_tile_band<D>(ldsK[buf], ldsV[buf], sub, kvs, len, myq, mylo, c2,
                       qfrag, ot, m, l, lq, hi);
    }
  };

  int buf = 0;
  load_tile(ph.begin);     // ph.begin <= q0_blk < len
  int64_t kv0 = ph.begin;
  for (; kv0 < ph.head_end; kv0 += 64) {
    write_tile(buf);
    __syncthreads();
    if (kv0 + 64 < ph.end) load_tile(kv0 + 64);
    masked_tile(buf, kv0);
    buf ^= 1;
  }
  for (; kv0 < ph.bulk_end; kv0 += 64) {
    write_tile(buf);
    __syncthreads();
    if (kv0 + 64 < ph.end) load_tile(kv0 + 64);
#pragma unroll
    for (int sub = 0; sub < 64; sub += 32)
      fwd_tile<false, false, D>(ldsK[buf], ldsV[buf], sub, kv0 + sub, len,
                                myq, c2, 1, qfrag, ot, m, l, lq, hi, nullptr,
                                0, 0u, 0u, 0u, 0, 1.f);
    buf ^= 1;
  }
  for (; kv0 < ph.end; kv0 += 64) {
    write_tile(buf);
    __syncthreads();
    if (kv0 + 64 < ph.end) load_tile(kv0 + 64);
    masked_tile(buf, kv0);
    buf ^= 1;
  }

  {
    unsigned int a, c;
    both_halves(__builtin_bit_cast(unsigned int, l), a, c);
    l = __builtin_bit_cast(float, a) + __builtin_bit_cast(float, c);
  }
  const float inv_l = 1.f / l;
  // O leaves through the freed K buffers as whole rows; every wave of the
  // block reaches both barriers
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

// dQ: attn_bwd_dq_gqa_kernel's causal path (direct two-barrier staging,
// delta published per query head) over the forward's three phases
template <int D>
__global__ __launch_bounds__(256, D == 64 ? 3 : 2)
void attn_bwd_dq_band_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, const short* __restrict__ dout,
    const float* __restrict__ lse, float* __restrict__ delta,
    short* __restrict__ dq, const short* __restrict__ out, int64_t seq,
    float scale, int64_t heads, int64_t group, int64_t in_sb, int64_t in_sh,
    int64_t in_ss, int64_t kv_sb, int64_t kv_sh, int64_t kv_ss,
    int64_t do_sb, int64_t do_sh, int64_t do_ss, int64_t g_sb, int64_t g_sh,
    int64_t g_ss, int64_t o_sb, int64_t o_sh, int64_t o_ss,
    const int* __restrict__ seqlens, const int* __restrict__ kv_lo,
    int64_t bound_sb) {
  __shared__ __attribute__((aligned(16))) short ldsK[64][img_pitch<D>()];
  __shared__ __attribute__((aligned(16))) short ldsVr[64][img_pitch<D>()];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int hi = lane >> 5;
  const int lq = lane & 31;
  const BlockPos pos = block_pos_band((unsigned int)group);
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
  const int* lo_row = kv_lo + b * bound_sb;

  const int64_t qrow = myq < len ? myq : len - 1;
  const int mylo = (int)lo_at(lo_row, qrow);
  const int64_t wave_lo = uniform(lo_at(lo_row, active ? q0 : len - 1));
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
  const KvPhases ph = kv_phases(lo_row, q0_blk, len);

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
  const int64_t wave_kv_end = q0 + 32 < len ? q0 + 32 : len;
  auto masked_tile = [&](int64_t kv0) {
    if (!active) return;
#pragma unroll
    for (int sub = 0; sub < 64; sub += 32) {
      const int64_t kvs = kv0 + sub;
      if (kvs >= wave_kv_end) break;
      if (kvs + 32 <= wave_lo) continue;
      dq_tile_band<D>(&ldsK[0][0], &ldsVr[0][0], sub, kvs, len, myq, mylo,
                      scale, mylse, mydelta, qfrag, dofrag, dqt, lq, hi);
    }
  };
  int64_t kv0 = ph.begin;
  for (; kv0 < ph.head_end; kv0 += 64) {
    stage_kv64(kv0);
    masked_tile(kv0);
  }
  for (; kv0 < ph.bulk_end; kv0 += 64) {
    stage_kv64(kv0);
#pragma unroll
    for (int sub = 0; sub < 64; sub += 32)
      dq_tile_tr<false, false, D>(&ldsK[0][0], &ldsVr[0][0], sub, kv0 + sub,
                                  len, myq, scale, 1, mylse, mydelta, qfrag,
                                  dofrag, dqt, lq, hi, nullptr, 0, 1.f);
  }
  for (; kv0 < ph.end; kv0 += 64) {
    stage_kv64(kv0);
    masked_tile(kv0);
  }

  if (!active || myq >= len) return;
#pragma unroll
  for (int dj = 0; dj < D / 32; ++dj)
    store_acc_bf16(dqb + myq * g_ss + dj * 32, dqt[dj], hi);
}

// kv-parallel backward: attn_bwd_kv_gqa_kernel's causal path (direct
// staging, the group's heads summed in registers in ascending order, one
// writer per output row) with an upper bound on the q loop.  Per head of
// the group: the DIAGONAL chunks, BULK chunks while every key of the
// block sees the whole chunk, a masked TAIL up to the last key's q_hi.
template <bool DK, int D>
__global__ __launch_bounds__(256, DK ? (D == 64 ? 3 : 2)
                                     : (D == 64 ? 4 : 3))
void attn_bwd_kv_band_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, const short* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    short* __restrict__ dkv, int64_t seq, float scale, int64_t heads,
    int64_t group, int64_t in_sb, int64_t in_sh, int64_t in_ss,
    int64_t kv_sb, int64_t kv_sh, int64_t kv_ss, int64_t do_sb,
    int64_t do_sh, int64_t do_ss, int64_t g_sb, int64_t g_sh, int64_t g_ss,
    const int* __restrict__ seqlens, const int* __restrict__ q_hi,
    int64_t bound_sb) {
  constexpr int PITCH = img_pitch<D>();
  constexpr int NC = DK ? 2 : 1;   // row constants: -lse/scale (, -delta)
  __shared__ __attribute__((aligned(16))) short ldsQ[64][PITCH];
  __shared__ __attribute__((aligned(16))) short ldsDO[64][PITCH];
  __shared__ __attribute__((aligned(16))) float ldsL[NC][64];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int hi = lane >> 5;
  const int lkv = lane & 31;
  const int64_t kv_heads = heads / group;
  const int64_t b = blockIdx.x / kv_heads, kvh = blockIdx.x % kv_heads;
  const int64_t kv0_blk = (int64_t)blockIdx.y * 128;
  const int64_t kv0 = kv0_blk + wave * 32;
  const int64_t len = sample_len(seqlens, b, seq);
  const int64_t mykv = kv0 + lkv;
  const int64_t goff = b * g_sb + kvh * g_sh + mykv * g_ss;
  if (mykv >= len && mykv < seq) zero_row<D>(dkv + goff, hi);
  if (kv0_blk >= len) return;
  const bool active = kv0 < len;
  const int* hi_row = q_hi + b * bound_sb;

  const int64_t kvrow = mykv < len ? mykv : len - 1;
  const int myhi = (int)hi_at(hi_row, kvrow, len);
  // the last key of the block (of the wave) holds the maximum
  const int64_t blk_last = kv0_blk + 127 < len ? kv0_blk + 127 : len - 1;
  const int64_t wave_last = kv0 + 31 < len ? kv0 + 31 : len - 1;
  const int64_t blk_q_end = uniform(hi_at(hi_row, blk_last, len));
  const int64_t wave_q_end = uniform(hi_at(hi_row, wave_last, len));
  const int64_t bulk_end =
      uniform(hi_at(hi_row, kv0_blk, len)) & ~(int64_t)63;
  const int64_t kvoff = b * kv_sb + kvh * kv_sh + kvrow * kv_ss + hi * 8;
  bf16x8 kfrag[D / 16], vfrag[D / 16];
#pragma unroll
  for (int c = 0; c < D / 16; ++c) {
    kfrag[c] = *reinterpret_cast<const bf16x8*>(k + kvoff + 16 * c);
    if (DK) vfrag[c] = *reinterpret_cast<const bf16x8*>(v + kvoff + 16 * c);
  }

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
  auto stage_q64 = [&](int64_t g, int64_t q0) {
    __syncthreads();
    if (wave < NC) {
      const int64_t qr = q0 + lane;
      const float* p = (wave == 0 ? lseg : dltg) + g * seq;
      ldsL[wave][lane] =
          p[qr < len ? qr : len - 1] * (wave == 0 ? neg_inv_scale : -1.f);
    }
    const short* qp = qg + g * in_sh;
    const short* dop = dog + g * do_sh;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      int64_t qr = q0 + stage_row + half * 32;
      if (qr >= len) qr = len - 1;
#pragma unroll
      for (int s = 0; s < D / 64; ++s) {
        *reinterpret_cast<bf16x8*>(
            img_at<D>(ldsQ, stage_row + half * 32, stage_seg + s * 64)) =
            *reinterpret_cast<const bf16x8*>(
                qp + qr * in_ss + stage_seg + s * 64);
        *reinterpret_cast<bf16x8*>(
            img_at<D>(ldsDO, stage_row + half * 32, stage_seg + s * 64)) =
            *reinterpret_cast<const bf16x8*>(
                dop + qr * do_ss + stage_seg + s * 64);
      }
    }
    __syncthreads();
  };
  auto masked_tile = [&](int sub, int64_t q0s) {
    if constexpr (DK)
      dk_tile_band<D>(&ldsQ[0][0], &ldsDO[0][0], &ldsL[0][sub],
                      &ldsL[NC - 1][sub], sub, q0s, len, mykv, myhi, scale,
                      kfrag, vfrag, acc, lkv, hi);
    else
      dv_tile_band<D>(&ldsQ[0][0], &ldsDO[0][0], &ldsL[0][sub], sub, q0s,
                      len, mykv, myhi, scale, kfrag, acc, lkv, hi);
  };
  auto plain_tile = [&](int sub, int64_t q0s) {
    if constexpr (DK)
      dk_tile_tr<false, false, D>(&ldsQ[0][0], &ldsDO[0][0], &ldsL[0][sub],
                                  &ldsL[NC - 1][sub], sub, q0s, len, mykv,
                                  scale, 1, kfrag, vfrag, acc, lkv, hi,
                                  nullptr, 0, 1.f);
    else
      dv_tile_tr<false, false, D>(&ldsQ[0][0], &ldsDO[0][0], &ldsL[0][sub],
                                  sub, q0s, len, mykv, scale, 1, kfrag, acc,
                                  lkv, hi, nullptr, 0, 1.f);
  };

  // blk_q_end <= len; kv0_blk < blk_q_end
  const int64_t diag_end =
      kv0_blk + 128 < blk_q_end ? kv0_blk + 128 : blk_q_end;
  for (int64_t g = 0; g < group; ++g) {
    int64_t q0 = kv0_blk;
    for (; q0 < diag_end; q0 += 64) {
      stage_q64(g, q0);
      if (!active) continue;
#pragma unroll
      for (int sub = 0; sub < 64; sub += 32) {
        const int64_t q0s = q0 + sub;
        if (q0s >= diag_end || q0s >= wave_q_end || q0s + 31 < kv0)
          continue;
        masked_tile(sub, q0s);
      }
    }
    for (; q0 + 63 < bulk_end; q0 += 64) {
      stage_q64(g, q0);
#pragma unroll
      for (int sub = 0; sub < 64; sub += 32)
        plain_tile(sub, q0 + sub);
    }
    for (; q0 < blk_q_end; q0 += 64) {
      stage_q64(g, q0);
      if (!active) continue;
#pragma unroll
      for (int sub = 0; sub < 64; sub += 32) {
        const int64_t q0s = q0 + sub;
        if (q0s >= wave_q_end) break;
        masked_tile(sub, q0s);
      }
    }
  }
  if (!active || mykv >= len) return;
#pragma unroll
  for (int dj = 0; dj < D / 32; ++dj)
    store_acc_bf16(dkv + goff + dj * 32, acc[dj], hi);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

}  // namespace

extern "C" {

void epl_attn_fwd_band(const void* q, const void* k, const void* v,
                       void* out, float* lse, int64_t batch_heads,
                       int64_t seq, float scale, int64_t heads,
                       int64_t kv_heads, int64_t head_dim,
                       const int64_t* in_strides, const int64_t* kv_strides,
                       const int64_t* o_strides, const int* seqlens,
                       const int* kv_lo, int64_t bound_sb,
                       hipStream_t stream) {
  const int64_t group = heads / kv_heads;
  const dim3 grid((unsigned)batch_heads, (unsigned)((seq + 127) / 128));
#define FWD_BAND_ARGS                                                    \
  reinterpret_cast<const short*>(q), reinterpret_cast<const short*>(k),  \
    reinterpret_cast<const short*>(v), reinterpret_cast<short*>(out),  \
    lse, seq, scale, heads, group, in_strides[0], in_strides[1],       \
    in_strides[2], kv_strides[0], kv_strides[1], kv_strides[2],        \
    o_strides[0], o_strides[1], o_strides[2], seqlens, kv_lo, bound_sb
  if (head_dim == 128)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(attn_fwd_band_kernel<128>), grid,
                       dim3(256), 0, stream, FWD_BAND_ARGS);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(attn_fwd_band_kernel<64>), grid,
                       dim3(256), 0, stream, FWD_BAND_ARGS);
#undef FWD_BAND_ARGS
}

void epl_attn_bwd_band(const void* q, const void* k, const void* v,
                       const void* out, const void* dout, const float* lse,
                       float* delta_ws, void* dq, void* dk, void* dv,
                       int64_t batch_heads, int64_t seq, float scale,
                       int64_t heads, int64_t kv_heads, int64_t head_dim,
                       const int64_t* in_strides, const int64_t* kv_strides,
                       const int64_t* o_strides, const int64_t* do_strides,
                       const int64_t* g_strides, const int64_t* gkv_strides,
                       const int* seqlens, const int* kv_lo,
                       const int* q_hi, int64_t bound_sb,
                       hipStream_t stream) {
  // dV over the B * Hkv grid -> dQ over the group-aware B * H grid
  // (publishes delta per query head) -> dK
  const int64_t group = heads / kv_heads;
  const unsigned n = (unsigned)((seq + 127) / 128);
  const dim3 kvgrid((unsigned)(batch_heads / group), n);
  const dim3 qgrid((unsigned)batch_heads, n);
#define KV_BAND_ARGS(res)                                                \
  reinterpret_cast<const short*>(q), reinterpret_cast<const short*>(k),  \
    reinterpret_cast<const short*>(v),                                 \
    reinterpret_cast<const short*>(dout), lse, delta_ws,               \
    reinterpret_cast<short*>(res), seq, scale, heads, group,           \
    in_strides[0], in_strides[1], in_strides[2], kv_strides[0],        \
    kv_strides[1], kv_strides[2], do_strides[0], do_strides[1],        \
    do_strides[2], gkv_strides[0], gkv_strides[1], gkv_strides[2],     \
    seqlens, q_hi, bound_sb
  auto launch = [&](auto d_c) {
    constexpr int D = decltype(d_c)::value;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(attn_bwd_kv_band_kernel<false, D>),
                       kvgrid, dim3(256), 0, stream, KV_BAND_ARGS(dv));
    hipLaunchKernelGGL(
        HIP_KERNEL_NAME(attn_bwd_dq_band_kernel<D>), qgrid, dim3(256), 0,
        stream, reinterpret_cast<const short*>(q),
        reinterpret_cast<const short*>(k),
        reinterpret_cast<const short*>(v),
        reinterpret_cast<const short*>(dout), lse, delta_ws,
        reinterpret_cast<short*>(dq), reinterpret_cast<const short*>(out),
        seq, scale, heads, group, in_strides[0], in_strides[1],
        in_strides[2], kv_strides[0], kv_strides[1], kv_strides[2],
        do_strides[0], do_strides[1], do_strides[2], g_strides[0],
        g_strides[1], g_strides[2], o_strides[0], o_strides[1],
        o_strides[2], seqlens, kv_lo, bound_sb);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(attn_bwd_kv_band_kernel<true, D>),
                       kvgrid, dim3(256), 0, stream, KV_BAND_ARGS(dk));
  };
  if (head_dim == 128)
    launch(std::integral_constant<int, 128>{});
  else
    launch(std::integral_constant<int, 64>{});
#undef KV_BAND_ARGS
}

}  // extern "C"
