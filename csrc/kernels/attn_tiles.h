// Shared device code of the flash attention kernels (attention.hip: MHA,
// attention_gqa.hip: grouped-query variants): vector types, MFMA fragment
// helpers, the row mask, block positions, the dropout RNG and the tile
// bodies of the forward and of the three backward kernels.  Everything is
// __forceinline__ in an anonymous namespace; a kernel file includes it
// once.  Design notes in attention.hip and docs/kernels.md.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "attn_block_order.h"
#include "attn_lds_image.h"

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using bf16x4 = __attribute__((ext_vector_type(4))) short;
using f32x16 = __attribute__((ext_vector_type(16))) float;
using i32x2 = __attribute__((ext_vector_type(2))) int;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned int;
using f32x2 = __attribute__((ext_vector_type(2))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using bf16v2 = __attribute__((ext_vector_type(2))) __bf16;

#define DEVI __device__ __forceinline__

namespace {

DEVI float bf2f(short u) {
  union { unsigned int i; float f; } v;
  v.i = ((unsigned int)(unsigned short)u) << 16;
  return v.f;
}

// C/D row for reg r, half hi of v_mfma_f32_32x32x16_bf16
DEVI int crow(int r, int hi) {
  return (r & 3) + 8 * (r >> 2) + 4 * hi;
}

// two floats -> packed bf16 pair, round-to-nearest-even, in one
// v_cvt_pk_bf16_f32
DEVI unsigned int cvt_pk_bf16(float a, float b) {
  f32x2 f = {a, b};
  return __builtin_bit_cast(unsigned int,
                            __builtin_convertvector(f, bf16v2));
}

// assemble the P^T mfma operand from 8 f32 scores (p[0..7] at rows
// crow(0..7, hi)): returns bf16x8 with element j = P at kv = hi*8+j.
DEVI bf16x8 assemble_pfrag(const float* p) {
  unsigned int c0 = cvt_pk_bf16(p[0], p[1]);
  unsigned int c1 = cvt_pk_bf16(p[2], p[3]);
  unsigned int c2 = cvt_pk_bf16(p[4], p[5]);
  unsigned int c3 = cvt_pk_bf16(p[6], p[7]);
  i32x2 r = __builtin_amdgcn_permlane32_swap((int)c0, (int)c2, false, false);
  i32x2 s = __builtin_amdgcn_permlane32_swap((int)c1, (int)c3, false, false);
  union { unsigned int d[4]; bf16x8 v; } out;
  out.d[0] = (unsigned int)r[0];
  out.d[1] = (unsigned int)s[0];
  out.d[2] = (unsigned int)r[1];
  out.d[3] = (unsigned int)s[1];
  return out.v;
}

// dual-use LDS image (row reads + transposed reads) of the backward's
// tile bodies and of the forward's V tile: layout and fragment readers in
// attn_lds_image.h
using attn_img::img_off;
using attn_img::img_pitch;
using attn_img::tr_frag;

// staging-store address of columns col..col+7 (col % 8 == 0) of a row of
// the dual-use image
template <int D>
DEVI short* img_at(short (&img)[64][img_pitch<D>()], int row, int col) {
  return &img[0][0] + img_off<D>(row, col >> 3);
}

// the 16 per-row constants of one lane's accumulator rows
// (crow(r, hi) = four consecutive rows per r>>2): four ds_read_b128,
// delivered as an accumulator so an MFMA chain can start from them
DEVI f32x16 load_rowconst(const float* c32, int hi) {
  f32x16 out;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(c32 + 8 * g + 4 * hi);
    out[4 * g + 0] = v[0];
    out[4 * g + 1] = v[1];
    out[4 * g + 2] = v[2];
    out[4 * g + 3] = v[3];
  }
  return out;
}

// MASKED tiles: element (qg, mykv) of tile row c = crow(r, hi),
// qg = q0 + c, is masked under the condition qg >= seq ||
// (causal && mykv > qg) || mykv >= seq, held as two 32-bit bounds:
// masked <=> c < lo || c >= hi_
struct RowMask {
  int lo, hi_;
  DEVI RowMask(int64_t q0, int64_t seq, int64_t mykv, int causal) {
    const int64_t rows = seq - q0;
    hi_ = mykv >= seq ? 0 : (rows < 32 ? (int)rows : 32);
    const int64_t d = mykv - q0;
    lo = (causal && d > 0) ? (d < 32 ? (int)d : 32) : 0;
  }
  DEVI bool masked(int c) const { return c < lo || c >= hi_; }
};

// epilogue: one lane's 16 accumulator rows of a 32-wide column block,
// rows crow(r, hi) -> four packed 8-byte stores
DEVI void store_acc_bf16(short* p, const f32x16& acc, int hi) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    u32x2 v = {cvt_pk_bf16(acc[4 * g], acc[4 * g + 1]),
               cvt_pk_bf16(acc[4 * g + 2], acc[4 * g + 3])};
    *reinterpret_cast<u32x2*>(p + 8 * g + 4 * hi) = v;
  }
}

// padded batches: sample b holds len = clamp(seqlens[b], 0, seq) valid
// leading rows; the rest is right padding.  A dense call (no seqlens)
// has len = seq.  The kernels use len wherever seq is a BOUND and keep
// seq wherever it is a PITCH (lse/delta rows, mask words, the grid).
// The value is block-uniform (it depends on bh alone); readfirstlane says
// so to the compiler, which otherwise holds len per lane in VGPRs and
// compares on the VALU (8 spilled dwords in the d64 dropout dV/dK).
DEVI int64_t sample_len(const int* seqlens, int64_t b, int64_t seq) {
  if (seqlens == nullptr) return seq;
  const int64_t n = __builtin_amdgcn_readfirstlane(seqlens[b]);
  return n < 0 ? 0 : (n > seq ? seq : n);
}

// this workgroup's batch-head and 128-row block.  Causal grids carry bh
// on x and the blocks on y (longest-first packing, see attn_fwd_kernel;
// `descending`: the q-parallel kernels take their longest block, the
// last one, first).  Non-causal grids carry the blocks on x and bh on y
// and take the XCD-local order of attn_block_order.h.  Block-uniform.
struct BlockPos {
  int64_t bh, blk;
};
DEVI BlockPos block_pos(int causal, bool descending) {
  if (causal)
    return {(int64_t)blockIdx.x,
            descending ? (int64_t)gridDim.y - 1 - blockIdx.y
                       : (int64_t)blockIdx.y};
  const attn_order::Block b =
      attn_order::block_of(blockIdx.x, blockIdx.y, gridDim.x, gridDim.y);
  return {(int64_t)b.bh, (int64_t)b.blk};
}

// padded rows are written as exact zeros: one lane's share of an output
// row (the columns store_acc_bf16 covers for this hi)
template <int D>
DEVI void zero_row(short* p, int hi) {
  const u32x2 z = {0u, 0u};
#pragma unroll
  for (int j = 0; j < D / 32; ++j)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<u32x2*>(p + j * 32 + 8 * g + 4 * hi) = z;
}

// ----------------------------------------------------------------------------
// philox4x32-10 counter-based RNG for in-kernel attention dropout.
// One call yields 16 bytes = the 16 Bernoulli draws of one lane's
// 32-key sub-tile (byte u >= thresh keeps; p is quantized to 1/256 —
// documented in ops/attention.py).  The keep-mask is packed into a
// [bh, seq, ceil(seq/32)] uint32 tensor during the FORWARD; the three
// backward kernels re-read bits instead of re-running philox.
// ----------------------------------------------------------------------------
DEVI void philox_round(unsigned int& c0, unsigned int& c1,
                       unsigned int& c2, unsigned int& c3,
                       unsigned int k0, unsigned int k1) {
  const unsigned int hi0 = __umulhi(0xD2511F53u, c0);
  const unsigned int lo0 = 0xD2511F53u * c0;
  const unsigned int hi1 = __umulhi(0xCD9E8D57u, c2);
  const unsigned int lo1 = 0xCD9E8D57u * c2;
  c0 = hi1 ^ c1 ^ k0;
  c1 = lo1;
  c2 = hi0 ^ c3 ^ k1;
  c3 = lo0;
}

DEVI void philox4x32(unsigned int c0, unsigned int c1, unsigned int c2,
                     unsigned int c3, unsigned int k0, unsigned int k1,
                     unsigned int out[4]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    philox_round(c0, c1, c2, c3, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the value of the partner lane (l ^ 32) by v_permlane32_swap: swapping a
// register with itself leaves the low half's value in one result and the
// high half's in the other, in every lane.  EXEC all ones.
DEVI void both_halves(unsigned int x, unsigned int& lo, unsigned int& hi_) {
  const i32x2 r = __builtin_amdgcn_permlane32_swap((int)x, (int)x, false,
                                                   false);
  lo = (unsigned int)r[0];
  hi_ = (unsigned int)r[1];
}

// deferred rescale: the running max m moves only when some row of the
// wave has grown past it by more than this many powers of two, so P
// stays <= 2^kRescaleThr (docs/kernels.md)
constexpr float kRescaleThr = 8.f;

// one 32-key sub-tile of the fwd online-softmax loop: the S products, one
// max exchange, one rescale decision, the exponentials, the PV products.
//  * m and the maxima are RAW accumulator values (scale > 0 commutes
//    with max); c2 = scale * log2(e) is folded into the one fma that
//    feeds v_exp_f32, and lse is put back into score units in the
//    epilogue.
//  * l is this lane's PARTIAL row sum: the partner lane (l ^ 32) applies
//    the same alpha throughout, so the halves add exactly in the epilogue.
//  * the rescale of ot and l is a wave-uniform branch on a vote, taken
//    before the first exponential of the step; on the other path m keeps
//    its stale value, so l, ot and lse always belong to the same m.
// MASKED adds the seq-bound + causal-diagonal masking (bulk tiles skip
// all of it); DROP generates + applies + publishes the dropout keep-mask
// per 32-key sub-tile (the normalizer l accumulates UNDROPPED exp values,
// so lse and the backward's P are dropout-free; O accumulates
// P*keep/(1-p)*V).  V^T operands come straight from the row image by
// ds_read_b64_tr_b16 (tr_frag: EXEC all ones, so every caller sits in
// wave-uniform control flow).
template <bool MASKED, bool DROP, int D>
DEVI void fwd_tile(const short (&ldsK)[64][D + 8], const short* imgV,
                   int sub, int64_t kvs, int64_t seq, int64_t myq,
                   float c2, int causal, const bf16x8 (&qfrag)[D / 16],
                   f32x16 (&ot)[D / 32], float& m, float& l, int lq,
                   int hi, unsigned int* maskrow, int64_t mask_w,
                   unsigned int seed0, unsigned int seed1,
                   unsigned int bh32, int drop_thresh, float inv_keep) {
  f32x16 st = {};
#pragma unroll
  for (int c = 0; c < D / 16; ++c) {
    bf16x8 kfrag =
        *reinterpret_cast<const bf16x8*>(&ldsK[sub + lq][hi * 8 + 16 * c]);
    st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfrag, qfrag[c], st, 0, 0,
                                                 0);
  }
  float s[16];
  float tile_max = -1e30f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float sv = st[r];
    if (MASKED) {
      const int64_t kvg = kvs + crow(r, hi);
      if (kvg >= seq || (causal && kvg > myq)) sv = -1e30f;
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
    s[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], c2, nmc));
    rowsum += s[r];
  }
  l += rowsum;
  if (DROP) {
    unsigned int rnd[4];
    philox4x32((unsigned int)myq,
               (unsigned int)(kvs >> 5) * 2u + (unsigned int)hi,
               bh32, 0x2E1B2137u, seed0, seed1, rnd);
    unsigned int mybits = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const unsigned int byte = (rnd[r >> 2] >> ((r & 3) * 8)) & 0xFFu;
      const bool keep = (int)byte >= drop_thresh;
      s[r] = keep ? s[r] * inv_keep : 0.f;
      mybits |= (unsigned int)keep << crow(r, hi);
    }
    unsigned int wlo, whi;
    both_halves(mybits, wlo, whi);
    if (hi == 0 && myq < seq)
      maskrow[myq * mask_w + (kvs >> 5)] = wlo | whi;
  }
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

// ----------------------------------------------------------------------------
// Tile bodies: one 32-row q sub-tile (`sub` selects the half of the
// 64-row staged chunk) of the dV or dK accumulation.
//  * Q/dO live in the dual-use image (img_off): row fragments by
//    ds_read_b128, each transposed fragment by two ds_read_b64_tr_b16;
//  * lse (and delta) of the chunk's 64 rows are staged in LDS with the
//    chunk and read as four ds_read_b128;
//  * bf16 rounding is v_cvt_pk_bf16_f32.
// lseL/dltL point at the 32 row constants of this sub-tile, staged as
// -lse/scale and -delta so the S and dP chains start from them and
// P = exp2(scale*log2(e) * S') needs no subtraction; rows past seq hold
// the clamped row's value.
// DROP, dV = P_d^T dO: P is masked+rescaled with the forward's keep bits
// (bit mykv&31 of the mask word of row qg — one broadcast word load per
// row).  DROP, dK mirrors dq_tile_tr: P undropped, the dO.V term
// masked+rescaled.
// ----------------------------------------------------------------------------
template <bool MASKED, bool DROP, int D>
DEVI void dv_tile_tr(const short* imgQ, const short* imgDO,
                     const float* lseL, int sub, int64_t q0, int64_t seq,
                     int64_t mykv, float scale, int causal,
                     const bf16x8 (&kfrag)[D / 16], f32x16 (&dvt)[D / 32],
                     int lkv, int hi, const unsigned int* maskrow,
                     int64_t mask_w, float inv_keep) {
  // row constants as the initial accumulator: S' = Q K^T - lse/scale
  f32x16 st = load_rowconst(lseL, hi);
#pragma unroll
  for (int c = 0; c < D / 16; ++c) {
    bf16x8 qf = *reinterpret_cast<const bf16x8*>(
        imgQ + img_off<D>(sub + lkv, 2 * c + hi));
    st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf, kfrag[c], st, 0, 0, 0);
  }
  const float c2 = scale * 1.44269504088896341f;   // P = exp2(c2 * S')
  const RowMask rm(q0, seq, mykv, causal);
  float p[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    if (MASKED)
      p[r] = rm.masked(crow(r, hi)) ? 0.f
                                    : __builtin_amdgcn_exp2f(st[r] * c2);
    else
      p[r] = __builtin_amdgcn_exp2f(st[r] * c2);
    if (DROP) {
      const int64_t qg = q0 + crow(r, hi);
      const int64_t qgc = qg < seq ? qg : seq - 1;
      const int64_t kvc = mykv < seq ? mykv : seq - 1;
      const unsigned int w = maskrow[qgc * mask_w + (kvc >> 5)];
      p[r] *= ((w >> (kvc & 31)) & 1u) ? inv_keep : 0.f;
    }
  }
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

template <bool MASKED, bool DROP, int D>
DEVI void dk_tile_tr(const short* imgQ, const short* imgDO,
                     const float* lseL, const float* dltL, int sub,
                     int64_t q0, int64_t seq, int64_t mykv, float scale,
                     int causal, const bf16x8 (&kfrag)[D / 16],
                     const bf16x8 (&vfrag)[D / 16], f32x16 (&dkt)[D / 32],
                     int lkv, int hi, const unsigned int* maskrow,
                     int64_t mask_w, float inv_keep) {
  // row constants as the initial accumulators: S' = Q K^T - lse/scale
  // and dP' = dO V^T - delta.  Dropout rescales dP before the
  // subtraction, so DROP keeps delta apart.
  f32x16 st = load_rowconst(lseL, hi);
  f32x16 dpt = {};
  if (!DROP) dpt = load_rowconst(dltL, hi);
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
  const RowMask rm(q0, seq, mykv, causal);
  float ds[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float dp = dpt[r];
    if (DROP) {
      const int64_t qg = q0 + crow(r, hi);
      const int64_t qgc = qg < seq ? qg : seq - 1;
      const int64_t kvc = mykv < seq ? mykv : seq - 1;
      const unsigned int w = maskrow[qgc * mask_w + (kvc >> 5)];
      dp *= ((w >> (kvc & 31)) & 1u) ? inv_keep : 0.f;
      dp += dltL[crow(r, hi)];
    }
    if (MASKED)
      ds[r] = rm.masked(crow(r, hi))
                  ? 0.f
                  : __builtin_amdgcn_exp2f(st[r] * c2) * dp * scale;
    else
      ds[r] = __builtin_amdgcn_exp2f(st[r] * c2) * dp * scale;
  }
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

// one 32-key sub-tile (of the 64-row staged chunk) of the dQ loop; the
// row constants (mylse, mydelta) are lane-local.
// DROP: dS = P o (dP_d o M/(1-p) - D) — P stays undropped, the V^T dO
// term is masked+rescaled with the forward's published keep bits.
template <bool MASKED, bool DROP, int D>
DEVI void dq_tile_tr(const short* imgK, const short* imgV, int sub,
                     int64_t kv0, int64_t seq, int64_t myq, float scale,
                     int causal, float mylse, float mydelta,
                     const bf16x8 (&qfrag)[D / 16],
                     const bf16x8 (&dofrag)[D / 16],
                     f32x16 (&dqt)[D / 32], int lq, int hi,
                     const unsigned int* maskrow, int64_t mask_w,
                     float inv_keep) {
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
  unsigned int mword = 0;
  if (DROP) {
    const int64_t qc = myq < seq ? myq : seq - 1;
    mword = maskrow[qc * mask_w + (kv0 >> 5)];
  }
  float ds[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float pv = __expf(st[r] * scale - mylse);
    if (MASKED) {
      const int64_t kvg = kv0 + crow(r, hi);
      if (myq >= seq || kvg >= seq || (causal && kvg > myq)) pv = 0.f;
    }
    float dp = dpt[r];
    if (DROP)
      dp *= ((mword >> crow(r, hi)) & 1u) ? inv_keep : 0.f;
    ds[r] = pv * (dp - mydelta) * scale;
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

}  // namespace
