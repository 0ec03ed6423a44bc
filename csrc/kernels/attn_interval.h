// Interval flash attention for gfx950: bidirectional packed documents,
// symmetric local windows, prefix-LM masks.  Query row i sees one
// contiguous interval of keys [kv_lo[i], kv_hi[i]) and key j is seen by one
// contiguous interval of queries [q_lo[j], q_hi[j]); all four bounds are
// non-decreasing along the sequence (ops/attention.py: interval_bounds).
// The band kernels (attention_band.hip) are the special case with the upper
// side hard-wired to the diagonal; here both sides are data.  Three
// kernels, bf16, d64 / d128, no dlse, on the GQA signature (G = 1 is MHA)
// plus the int32 bound rows and one batch stride for them (bound_sb = 0:
// one row broadcast over the batch).  The templates live here and take a
// `bool DROP`; attention_interval.hip instantiates DROP = false and
// attention_interval_drop.hip DROP = true, each a translation unit of its
// own, so that the no-dropout instantiations (and the MHA, GQA and band
// ones) compile to the code they compiled to before dropout existed here:
// every dropout line sits under `if constexpr (DROP)`.
//
//  * the two sides of the problem are mirror images — rows bounded by
//    (kv_lo, kv_hi) over keys, keys bounded by (q_lo, q_hi) over rows — so
//    one `phases()` serves the q-parallel and the kv-parallel kernels: it
//    takes the block's first index and reads four scalars (readfirstlane,
//    as sample_len).  By monotonicity the first index holds the block's
//    minimum lower bound and the last valid one its maximum upper bound.
//  * three phases in ascending order of the streamed index: masked HEAD
//    tiles up to round_up64(lo[last]); branch-free BULK tiles, which every
//    row (key) of the block sees in full, up to min(hi[first], end) & ~63,
//    through the plain bodies of attn_tiles.h; a masked TAIL up to
//    hi[last].  A block whose head end is at or past its bulk end (every
//    document shorter than a block) has no bulk phase.
//  * inside the masked phases a wave skips the 32-wide sub-tiles below the
//    lower bound of its first row (key) or at or past the upper bound of
//    its last valid one; the tests are wave-uniform (tr_frag needs EXEC all
//    ones).
//  * every bound is clamped where it is read: a lower bound to [0, i], an
//    upper bound to [i + 1, len].  Values that break monotonicity give a
//    wrong visible set, never an access outside the sample's rows, and
//    every valid row keeps its own key, so no softmax row is empty.
//
// With trivial bounds (0 and S everywhere) the HEAD phase is empty, BULK
// and TAIL are the non-causal GQA kernels' two phases, and the results are
// their bits.
//
// DROP: the semantics and the philox keying of the MHA kernels
// (attn_tiles.h), with bh the QUERY head b * H + h.  The forward draws and
// publishes keep bits for the sub-tiles it visits (rows < len); the
// backward re-reads them and never runs philox.  The mask tensor is
// uninitialised memory outside those words, so every backward use of a bit
// only SELECTS between two finite factors (inv_keep or 0) and multiplies a
// term whose P is already an exact 0 wherever the word may be garbage.
//  * dQ: a lane owns a query row and needs one word per 32-key sub-tile;
//    the chunk's two words are loaded ahead of the staging barrier.
//  * dV / dK: a wave owns 32 keys aligned at 32 — one word per query row —
//    and the block's 128 keys are four consecutive words.  stage_q64
//    stages the chunk's 64 rows x 4 words of query head g with the Q / dO
//    chunk (one dword per thread, laid out [4][64]); a wave reads its 16
//    rows' words with four ds_read_b128, as load_rowconst reads lse.  The
//    DROP bodies of attn_tiles.h load the word from global memory per
//    accumulator row inside the tile, so the DROP bulk phase runs the
//    bodies below with the mask test compiled out instead.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

#include "attn_tiles.h"

namespace {

// the dropout arguments of a kernel: nothing without dropout
template <bool DROP>
struct IntervalDrop {};
template <>
struct IntervalDrop<true> {
  unsigned int* mask;   // [B * H, seq, mask_w] keep bits
  int64_t mask_w;       // ceil(seq / 32)
  unsigned int seed0, seed1;
  int thresh;           // a philox byte >= thresh keeps
  float inv_keep;
};

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                   \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// lower bound of index i (0 <= i < len), clamped to [0, i]
DEVI int64_t lo_at(const int* lo, int64_t i) {
  const int64_t x = lo[i];
  return x < 0 ? 0 : (x > i ? i : x);
}

// upper bound of index i (0 <= i < len), clamped to [i + 1, len]
DEVI int64_t hi_at(const int* hi, int64_t i, int64_t len) {
  const int64_t x = hi[i];
  return x <= i ? i + 1 : (x > len ? len : x);
}

DEVI int64_t uniform(int64_t x) {
  return __builtin_amdgcn_readfirstlane((int)x);
}

// the streamed loop of a block of indices [first, first + 128), first <
// len: chunks of 64 from `begin`; masked up to `head_end`, plain up to
// `bulk_end`, masked up to `end`.  begin <= first < end <= len, begin and
// bulk_end are multiples of 64, head_end <= end and bulk_end <= end hold
// for any bound values, so the three loops never leave [begin, end).
struct Phases {
  int64_t begin, head_end, bulk_end, end;
};
DEVI Phases phases(const int* lo_row, const int* hi_row, int64_t first,
                   int64_t len) {
  const int64_t last = first + 127 < len ? first + 127 : len - 1;
  Phases p;
  p.begin = uniform(lo_at(lo_row, first)) & ~(int64_t)63;
  p.end = uniform(hi_at(hi_row, last, len));
  const int64_t head = (uniform(lo_at(lo_row, last)) + 63) & ~(int64_t)63;
  p.head_end = head < p.end ? head : p.end;
  const int64_t vis = uniform(hi_at(hi_row, first, len));
  p.bulk_end = (vis < p.end ? vis : p.end) & ~(int64_t)63;
  return p;
}

// the wave's share of a masked chunk: its 32 indices from w0 see the
// streamed sub-tiles that intersect [lo, hi)
struct WaveSpan {
  int64_t lo, hi;
  DEVI bool skips(int64_t s0) const { return s0 + 32 <= lo || s0 >= hi; }
};
DEVI WaveSpan wave_span(const int* lo_row, const int* hi_row, int64_t w0,
                        int64_t len) {
  // an inactive wave (w0 >= len) never asks; give it the last row's span
  const int64_t first = w0 < len ? w0 : len - 1;
  const int64_t last = w0 + 31 < len ? w0 + 31 : len - 1;
  return {uniform(lo_at(lo_row, first)), uniform(hi_at(hi_row, last, len))};
}

// what a forward lane needs to draw and publish its keep bits: the mask
// row of its query head, the philox key and counter words, and whether its
// row is a valid one (only those publish)
template <bool DROP>
struct FwdDrop {};
template <>
struct FwdDrop<true> {
  unsigned int* word;   // mask word 0 of row myq
  unsigned int seed0, seed1, bh32, myq32;
  int thresh;
  float inv_keep;
  bool publish;         // hi == 0 && myq < len
};

// fwd_tile<true, DROP, D> (attn_tiles.h) with the interval mask
// kvg < mylo || kvg >= myhi (myhi <= len covers the sequence bound).  A
// row may have hidden sub-tiles before AND after its visible ones.  A
// hidden key's P is set to an exact 0 after the exponential, as in
// fwd_tile_band and for its reason: while a row has seen no key, m is
// still -1e30 and exp2((s - m) * c2) of a -1e30 score is 1, not 0; with P
// zeroed, l and ot of the row stay exact zeros until its first visible key
// sets m (its score exceeds -1e30 by more than kRescaleThr), and nothing
// relies on a rescale with alpha = 0.  After a row's first key the -1e30
// score alone gives an exact 0, so tiles in which nothing precedes the
// visible keys compute what fwd_tile<true> computes.  Dropout comes after
// that zero, in fwd_tile's words: l has the undropped sum by then.
template <bool DROP, int D>
DEVI void fwd_tile_interval(const short (&ldsK)[64][D + 8],
                            const short* imgV, int sub, int64_t kvs,
                            int mylo, int myhi, float c2,
                            const bf16x8 (&qfrag)[D / 16],
                            f32x16 (&ot)[D / 32], float& m, float& l,
                            int lq, int hi, const FwdDrop<DROP>& fd) {
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
  const int kv32 = (int)kvs;   // kvs < len <= seq < 2^31 (grid check)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float sv = st[r];
    const int kvg = kv32 + crow(r, hi);
    if (kvg < mylo || kvg >= myhi) {
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
  if constexpr (DROP) {
    unsigned int rnd[4];
    philox4x32(fd.myq32, (unsigned int)(kvs >> 5) * 2u + (unsigned int)hi,
               fd.bh32, 0x2E1B2137u, fd.seed0, fd.seed1, rnd);
    unsigned int mybits = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const unsigned int byte = (rnd[r >> 2] >> ((r & 3) * 8)) & 0xFFu;
      const bool keep = (int)byte >= fd.thresh;
      s[r] = keep ? s[r] * fd.inv_keep : 0.f;
      mybits |= (unsigned int)keep << crow(r, hi);
    }
    unsigned int wlo, whi;
    both_halves(mybits, wlo, whi);
    if (fd.publish) fd.word[kvs >> 5] = wlo | whi;
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

// dq_tile_tr<MASKED, DROP, D> with the interval mask; `dead` marks a lane
// whose query row is padding.  DROP: mword holds the keep bits of the
// lane's row for this sub-tile's 32 keys; a bit selects inv_keep or 0 for
// dP, which stays finite, and a hidden key's P = 0 then gives dS = 0
// whatever an unwritten word holds.  MASKED = false (DROP bulk tiles only)
// compiles the interval test out.
template <bool DROP, bool MASKED, int D>
DEVI void dq_tile_interval(const short* imgK, const short* imgV, int sub,
                           int64_t kv0, bool dead, int mylo, int myhi,
                           float scale, float mylse, float mydelta,
                           const bf16x8 (&qfrag)[D / 16],
                           const bf16x8 (&dofrag)[D / 16],
                           f32x16 (&dqt)[D / 32], int lq, int hi,
                           unsigned int mword, float inv_keep) {
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
  // a dead lane's interval is made empty once, outside the element loop
  const int lo = dead ? 0x7fffffff : mylo;
  const int kv32 = (int)kv0;
  float ds[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float pv = __expf(st[r] * scale - mylse);
    if constexpr (MASKED) {
      const int kvg = kv32 + crow(r, hi);
      if (kvg < lo || kvg >= myhi) pv = 0.f;
    }
    if constexpr (DROP) {
      float dp = dpt[r];
      dp *= ((mword >> crow(r, hi)) & 1u) ? inv_keep : 0.f;
      ds[r] = pv * (dp - mydelta) * scale;
    } else {
      ds[r] = pv * (dpt[r] - mydelta) * scale;
    }
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

// the non-causal RowMask of key mykv over the 32 query rows from q0 with
// both ends taken from the key's interval [mylo, myhi): still two 32-bit
// compares per element
DEVI RowMask interval_mask(int64_t q0, int64_t len, int64_t mykv, int mylo,
                           int myhi) {
  RowMask rm(q0, len, mykv, 0);
  const int64_t l = (int64_t)mylo - q0, h = (int64_t)myhi - q0;
  if (l > 0) rm.lo = l < 32 ? (int)l : 32;
  if (h < rm.hi_) rm.hi_ = h < 0 ? 0 : (int)h;
  return rm;
}

// the keep words of one lane's 16 accumulator rows from the [4][64] LDS
// image (w32: the wave's word column at the sub-tile's first row): four
// ds_read_b128, as load_rowconst
DEVI void load_rowwords(const unsigned int* w32, int hi,
                        unsigned int (&out)[16]) {
  using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(w32 + 8 * g + 4 * hi);
    out[4 * g + 0] = v[0];
    out[4 * g + 1] = v[1];
    out[4 * g + 2] = v[2];
    out[4 * g + 3] = v[3];
  }
}

// dv_tile_tr<MASKED, DROP, D> with the interval mask.  DROP: mwL points at
// the staged keep words of the sub-tile's 32 query rows for this wave's 32
// keys, bit lkv is this lane's key; P is multiplied by inv_keep or 0, so a
// masked P stays an exact 0 under any word.
template <bool DROP, bool MASKED, int D>
DEVI void dv_tile_interval(const short* imgQ, const short* imgDO,
                           const float* lseL, const unsigned int* mwL,
                           int sub, const RowMask& rm, float scale,
                           const bf16x8 (&kfrag)[D / 16],
                           f32x16 (&dvt)[D / 32], int lkv, int hi,
                           float inv_keep) {
  f32x16 st = load_rowconst(lseL, hi);
#pragma unroll
  for (int c = 0; c < D / 16; ++c) {
    bf16x8 qf = *reinterpret_cast<const bf16x8*>(
        imgQ + img_off<D>(sub + lkv, 2 * c + hi));
    st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf, kfrag[c], st, 0, 0, 0);
  }
  [[maybe_unused]] unsigned int mw[16];
  if constexpr (DROP) load_rowwords(mwL, hi, mw);
  const float c2 = scale * 1.44269504088896341f;   // P = exp2(c2 * S')
  float p[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    if constexpr (MASKED)
      p[r] = rm.masked(crow(r, hi)) ? 0.f
                                    : __builtin_amdgcn_exp2f(st[r] * c2);
    else
      p[r] = __builtin_amdgcn_exp2f(st[r] * c2);
    if constexpr (DROP) p[r] *= ((mw[r] >> lkv) & 1u) ? inv_keep : 0.f;
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

// dk_tile_tr<MASKED, DROP, D> with the interval mask.  Dropout rescales dP
// before the subtraction, so DROP starts the dP chain from zero and adds
// -delta (read like the keep words, as row constants) afterwards; dP stays
// finite under any word and the masked dS is an exact 0.
template <bool DROP, bool MASKED, int D>
DEVI void dk_tile_interval(const short* imgQ, const short* imgDO,
                           const float* lseL, const float* dltL,
                           const unsigned int* mwL, int sub,
                           const RowMask& rm, float scale,
                           const bf16x8 (&kfrag)[D / 16],
                           const bf16x8 (&vfrag)[D / 16],
                           f32x16 (&dkt)[D / 32], int lkv, int hi,
                           float inv_keep) {
  f32x16 st = load_rowconst(lseL, hi);
  f32x16 dpt = {};
  if constexpr (!DROP) dpt = load_rowconst(dltL, hi);
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
  float ds[16];
  if constexpr (DROP) {
    unsigned int mw[16];
    load_rowwords(mwL, hi, mw);
    const f32x16 dlt = load_rowconst(dltL, hi);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float dp = dpt[r];
      dp *= ((mw[r] >> lkv) & 1u) ? inv_keep : 0.f;
      dp += dlt[r];
      if constexpr (MASKED)
        ds[r] = rm.masked(crow(r, hi))
                    ? 0.f
                    : __builtin_amdgcn_exp2f(st[r] * c2) * dp * scale;
      else
        ds[r] = __builtin_amdgcn_exp2f(st[r] * c2) * dp * scale;
    }
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r)
      ds[r] = rm.masked(crow(r, hi))
                  ? 0.f
                  : __builtin_amdgcn_exp2f(st[r] * c2) * dpt[r] * scale;
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

// the [4][64] keep-word image of the kv-parallel kernels: only the DROP
// instantiations own the 1 KiB
template <bool DROP>
DEVI unsigned int* keep_word_lds() {
  if constexpr (DROP) {
    __shared__ __attribute__((aligned(16))) unsigned int words[4][64];
    return &words[0][0];
  } else {
    return nullptr;
  }
}

// the non-causal q-parallel grid dim3(n * G, B * Hkv) in the group-aware
// order of attn_block_order.h.  Every block's work is bounded by its own
// interval, so there is no longest-first order to keep.
DEVI BlockPos block_pos_interval(unsigned int group) {
  const attn_order::Block b = attn_order::block_of_group(
      blockIdx.x, blockIdx.y, gridDim.x / group, group, gridDim.y);
  return {(int64_t)b.bh, (int64_t)b.blk};
}

// forward: attn_fwd_gqa_kernel's non-causal path — the single-barrier
// double-buffered staging, the LDS epilogue — over the three phases.  The
// first staged tile, the prefetch guard and the buffer parity all count
// from ph.begin.
template <bool DROP, int D>
__global__ __launch_bounds__(256, D == 64 ? 3 : 2)
void attn_fwd_interval_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, short* __restrict__ out,
    float* __restrict__ lse, int64_t seq, float scale, int64_t heads,
    int64_t group, int64_t in_sb, int64_t in_sh, int64_t in_ss,
    int64_t kv_sb, int64_t kv_sh, int64_t kv_ss, int64_t o_sb, int64_t o_sh,
    int64_t o_ss, const int* __restrict__ seqlens,
    const int* __restrict__ kv_lo, const int* __restrict__ kv_hi,
    int64_t bound_sb, IntervalDrop<DROP> da) {
  __shared__ __attribute__((aligned(16))) short
      ldsV[2][64 * img_pitch<D>()];
  __shared__ __attribute__((aligned(16))) short ldsK[2][64][D + 8];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int hi = lane >> 5;
  const int lq = lane & 31;
  const BlockPos pos = block_pos_interval((unsigned int)group);
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
  const int* hi_row = kv_hi + b * bound_sb;

  const int64_t qrow = myq < len ? myq : len - 1;
  const int mylo = (int)lo_at(lo_row, qrow);
  const int myhi = (int)hi_at(hi_row, qrow, len);
  const WaveSpan span = wave_span(lo_row, hi_row, q0, len);
  bf16x8 qfrag[D / 16];
#pragma unroll
  for (int c = 0; c < D / 16; ++c)
    qfrag[c] = *reinterpret_cast<const bf16x8*>(
        qp + qrow * in_ss + hi * 8 + 16 * c);

  f32x16 ot[D / 32] = {};
  float m = -1e30f, l = 0.f;
  const float c2 = scale * 1.44269504088896341f;
  const Phases ph = phases(lo_row, hi_row, q0_blk, len);

  // the keep words of query head bh; a padded row never publishes, its
  // pointer stays on the clamped row
  FwdDrop<DROP> fd;
  [[maybe_unused]] unsigned int* maskrow = nullptr;
  if constexpr (DROP) {
    maskrow = da.mask + bh * seq * da.mask_w;
    fd.word = maskrow + qrow * da.mask_w;
    fd.seed0 = da.seed0;
    fd.seed1 = da.seed1;
    fd.bh32 = (unsigned int)bh;
    fd.myq32 = (unsigned int)myq;
    fd.thresh = da.thresh;
    fd.inv_keep = da.inv_keep;
    fd.publish = hi == 0 && myq < len;
  }

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
  // one masked 64-key tile: the wave's sub-tiles inside its span
  auto masked_tile = [&](int buf, int64_t kv0) {
    if (!active) return;
#pragma unroll
    for (int sub = 0; sub < 64; sub += 32) {
      const int64_t kvs = kv0 + sub;
      if (span.skips(kvs)) continue;
      fwd_tile_interval<DROP, D>(ldsK[buf], ldsV[buf], sub, kvs, mylo, myhi,
                                 c2, qfrag, ot, m, l, lq, hi, fd);
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
    for (int sub = 0; sub < 64; sub += 32) {
      // fwd_tile's DROP path draws, applies and publishes (rows < len) as
      // the masked body does: it writes the words and reads none
      if constexpr (DROP)
        fwd_tile<false, true, D>(ldsK[buf], ldsV[buf], sub, kv0 + sub, len,
                                 myq, c2, 0, qfrag, ot, m, l, lq, hi,
                                 maskrow, da.mask_w, da.seed0, da.seed1,
                                 (unsigned int)bh, da.thresh, da.inv_keep);
      else
        fwd_tile<false, false, D>(ldsK[buf], ldsV[buf], sub, kv0 + sub, len,
                                  myq, c2, 0, qfrag, ot, m, l, lq, hi,
                                  nullptr, 0, 0u, 0u, 0u, 0, 1.f);
    }
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

// dQ: attn_bwd_dq_gqa_kernel's non-causal path (direct two-barrier
// staging, delta published per query head) over the forward's phases
template <bool DROP, int D>
__global__ __launch_bounds__(256, D == 64 ? 3 : 2)
void attn_bwd_dq_interval_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, const short* __restrict__ dout,
    const float* __restrict__ lse, float* __restrict__ delta,
    short* __restrict__ dq, const short* __restrict__ out, int64_t seq,
    float scale, int64_t heads, int64_t group, int64_t in_sb, int64_t in_sh,
    int64_t in_ss, int64_t kv_sb, int64_t kv_sh, int64_t kv_ss,
    int64_t do_sb, int64_t do_sh, int64_t do_ss, int64_t g_sb, int64_t g_sh,
    int64_t g_ss, int64_t o_sb, int64_t o_sh, int64_t o_ss,
    const int* __restrict__ seqlens, const int* __restrict__ kv_lo,
    const int* __restrict__ kv_hi, int64_t bound_sb,
    IntervalDrop<DROP> da) {
  __shared__ __attribute__((aligned(16))) short ldsK[64][img_pitch<D>()];
  __shared__ __attribute__((aligned(16))) short ldsVr[64][img_pitch<D>()];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int hi = lane >> 5;
  const int lq = lane & 31;
  const BlockPos pos = block_pos_interval((unsigned int)group);
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
  const int* hi_row = kv_hi + b * bound_sb;

  const int64_t qrow = myq < len ? myq : len - 1;
  const int mylo = (int)lo_at(lo_row, qrow);
  const int myhi = (int)hi_at(hi_row, qrow, len);
  const WaveSpan span = wave_span(lo_row, hi_row, q0, len);
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
  const Phases ph = phases(lo_row, hi_row, q0_blk, len);

  // DROP: the keep words of the lane's (clamped) row for the chunk's two
  // sub-tiles, loaded ahead of the staging barrier; the word index is
  // clamped to the row (a chunk's second sub-tile may lie past the last
  // word, and is then past len: skipped or fully masked)
  [[maybe_unused]] unsigned int mword[2] = {0u, 0u};
  [[maybe_unused]] const unsigned int* mrow = nullptr;
  [[maybe_unused]] float inv_keep = 1.f;
  if constexpr (DROP) {
    mrow = da.mask + (bh * seq + qrow) * da.mask_w;
    inv_keep = da.inv_keep;
  }

  auto stage_kv64 = [&](int64_t kv0) {
    if constexpr (DROP) {
      const int64_t w0 = kv0 >> 5;
      mword[0] = mrow[w0];   // kv0 < len: a word of the row
      mword[1] = mrow[w0 + 1 < da.mask_w ? w0 + 1 : da.mask_w - 1];
    }
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
  const bool dead = myq >= len;
  auto masked_tile = [&](int64_t kv0) {
    if (!active) return;
#pragma unroll
    for (int sub = 0; sub < 64; sub += 32) {
      const int64_t kvs = kv0 + sub;
      if (span.skips(kvs)) continue;
      dq_tile_interval<DROP, true, D>(&ldsK[0][0], &ldsVr[0][0], sub, kvs,
                                      dead, mylo, myhi, scale, mylse,
                                      mydelta, qfrag, dofrag, dqt, lq, hi,
                                      mword[sub >> 5], inv_keep);
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
    for (int sub = 0; sub < 64; sub += 32) {
      if constexpr (DROP)
        dq_tile_interval<true, false, D>(&ldsK[0][0], &ldsVr[0][0], sub,
                                         kv0 + sub, dead, mylo, myhi, scale,
                                         mylse, mydelta, qfrag, dofrag, dqt,
                                         lq, hi, mword[sub >> 5], inv_keep);
      else
        dq_tile_tr<false, false, D>(&ldsK[0][0], &ldsVr[0][0], sub,
                                    kv0 + sub, len, myq, scale, 0, mylse,
                                    mydelta, qfrag, dofrag, dqt, lq, hi,
                                    nullptr, 0, 1.f);
    }
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

// kv-parallel backward: attn_bwd_kv_gqa_kernel's non-causal direct path
// (the group's heads summed in registers in ascending order, one writer
// per output row) with the q loop bounded on both sides by the keys'
// (q_lo, q_hi).  The three phases restart for each head of the group with
// the same bounds.
template <bool DROP, bool DK, int D>
__global__ __launch_bounds__(256, (DK ? (D == 64 ? 3 : 2)
                                      : (D == 64 ? 4 : 3)) -
                                         (DROP && (!DK || D == 64) ? 1 : 0))
void attn_bwd_kv_interval_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, const short* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    short* __restrict__ dkv, int64_t seq, float scale, int64_t heads,
    int64_t group, int64_t in_sb, int64_t in_sh, int64_t in_ss,
    int64_t kv_sb, int64_t kv_sh, int64_t kv_ss, int64_t do_sb,
    int64_t do_sh, int64_t do_ss, int64_t g_sb, int64_t g_sh, int64_t g_ss,
    const int* __restrict__ seqlens, const int* __restrict__ q_lo,
    const int* __restrict__ q_hi, int64_t bound_sb, IntervalDrop<DROP> da) {
  constexpr int PITCH = img_pitch<D>();
  constexpr int NC = DK ? 2 : 1;   // row constants: -lse/scale (, -delta)
  __shared__ __attribute__((aligned(16))) short ldsQ[64][PITCH];
  __shared__ __attribute__((aligned(16))) short ldsDO[64][PITCH];
  __shared__ __attribute__((aligned(16))) float ldsL[NC][64];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int hi = lane >> 5;
  const int lkv = lane & 31;
  // plain block_pos over the B * Hkv batch-kv-heads: the axes and the
  // order of the non-causal dV / dK grids
  const BlockPos pos = block_pos(0, false);
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
  const int* lo_row = q_lo + b * bound_sb;
  const int* hi_row = q_hi + b * bound_sb;

  const int64_t kvrow = mykv < len ? mykv : len - 1;
  const int mylo = (int)lo_at(lo_row, kvrow);
  const int myhi = (int)hi_at(hi_row, kvrow, len);
  const WaveSpan span = wave_span(lo_row, hi_row, kv0, len);
  const Phases ph = phases(lo_row, hi_row, kv0_blk, len);
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

  // DROP: thread t stages word t & 3 of the block's four (clamped to the
  // row's last word: such a word's keys are past len and masked) for chunk
  // row t >> 2 (clamped to len - 1, as Q and dO are), so four neighbours
  // read 16 consecutive bytes; wave w reads column w of the image
  unsigned int* ldsM = keep_word_lds<DROP>();
  [[maybe_unused]] const unsigned int* mwave = nullptr;
  [[maybe_unused]] const unsigned int* maskg = nullptr;
  [[maybe_unused]] int64_t mword_i = 0;
  [[maybe_unused]] float inv_keep = 1.f;
  if constexpr (DROP) {
    mwave = ldsM + wave * 64;
    maskg = da.mask + (b * heads + h0) * seq * da.mask_w;
    mword_i = (kv0_blk >> 5) + (threadIdx.x & 3);
    if (mword_i >= da.mask_w) mword_i = da.mask_w - 1;
    inv_keep = da.inv_keep;
  }

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
    if constexpr (DROP) {
      int64_t qr = q0 + (threadIdx.x >> 2);
      if (qr >= len) qr = len - 1;
      ldsM[(threadIdx.x & 3) * 64 + (threadIdx.x >> 2)] =
          maskg[(g * seq + qr) * da.mask_w + mword_i];
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
  auto masked_chunk = [&](int64_t q0) {
    if (!active) return;
#pragma unroll
    for (int sub = 0; sub < 64; sub += 32) {
      const int64_t q0s = q0 + sub;
      if (span.skips(q0s)) continue;
      const RowMask rm = interval_mask(q0s, len, mykv, mylo, myhi);
      if constexpr (DK)
        dk_tile_interval<DROP, true, D>(
            &ldsQ[0][0], &ldsDO[0][0], &ldsL[0][sub], &ldsL[NC - 1][sub],
            mwave + sub, sub, rm, scale, kfrag, vfrag, acc, lkv, hi,
            inv_keep);
      else
        dv_tile_interval<DROP, true, D>(
            &ldsQ[0][0], &ldsDO[0][0], &ldsL[0][sub], mwave + sub, sub, rm,
            scale, kfrag, acc, lkv, hi, inv_keep);
    }
  };
  auto plain_tile = [&](int sub, int64_t q0s) {
    if constexpr (DROP) {
      // every row of the sub-tile sees every key of the block: the mask
      // test is compiled out and rm is never read
      const RowMask rm(q0s, len, mykv, 0);
      if constexpr (DK)
        dk_tile_interval<true, false, D>(
            &ldsQ[0][0], &ldsDO[0][0], &ldsL[0][sub], &ldsL[NC - 1][sub],
            mwave + sub, sub, rm, scale, kfrag, vfrag, acc, lkv, hi,
            inv_keep);
      else
        dv_tile_interval<true, false, D>(
            &ldsQ[0][0], &ldsDO[0][0], &ldsL[0][sub], mwave + sub, sub, rm,
            scale, kfrag, acc, lkv, hi, inv_keep);
    } else if constexpr (DK) {
      dk_tile_tr<false, false, D>(&ldsQ[0][0], &ldsDO[0][0], &ldsL[0][sub],
                                  &ldsL[NC - 1][sub], sub, q0s, len, mykv,
                                  scale, 0, kfrag, vfrag, acc, lkv, hi,
                                  nullptr, 0, 1.f);
    } else {
      dv_tile_tr<false, false, D>(&ldsQ[0][0], &ldsDO[0][0], &ldsL[0][sub],
                                  sub, q0s, len, mykv, scale, 0, kfrag, acc,
                                  lkv, hi, nullptr, 0, 1.f);
    }
  };

  for (int64_t g = 0; g < group; ++g) {
    int64_t q0 = ph.begin;
    for (; q0 < ph.head_end; q0 += 64) {
      stage_q64(g, q0);
      masked_chunk(q0);
    }
    for (; q0 < ph.bulk_end; q0 += 64) {
      stage_q64(g, q0);
#pragma unroll
      for (int sub = 0; sub < 64; sub += 32)
        plain_tile(sub, q0 + sub);
    }
    for (; q0 < ph.end; q0 += 64) {
      stage_q64(g, q0);
      masked_chunk(q0);
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

// host launches, shared by the two translation units

template <bool DROP>
void launch_fwd_interval(const void* q, const void* k, const void* v,
                         void* out, float* lse, int64_t batch_heads,
                         int64_t seq, float scale, int64_t heads,
                         int64_t kv_heads, int64_t head_dim,
                         const int64_t* in_strides,
                         const int64_t* kv_strides,
                         const int64_t* o_strides, const int* seqlens,
                         const int* kv_lo, const int* kv_hi,
                         int64_t bound_sb, IntervalDrop<DROP> da,
                         hipStream_t stream) {
  const int64_t group = heads / kv_heads;
  const unsigned n = (unsigned)((seq + 127) / 128);
  const dim3 grid(n * (unsigned)group, (unsigned)(batch_heads / group));
#define FWD_INTERVAL_ARGS                                                \
  reinterpret_cast<const short*>(q), reinterpret_cast<const short*>(k),  \
    reinterpret_cast<const short*>(v), reinterpret_cast<short*>(out),  \
    lse, seq, scale, heads, group, in_strides[0], in_strides[1],       \
    in_strides[2], kv_strides[0], kv_strides[1], kv_strides[2],        \
    o_strides[0], o_strides[1], o_strides[2], seqlens, kv_lo, kv_hi,   \
    bound_sb, da
  if (head_dim == 128)
    hipLaunchKernelGGL(
        HIP_KERNEL_NAME(attn_fwd_interval_kernel<DROP, 128>), grid,
        dim3(256), 0, stream, FWD_INTERVAL_ARGS);
  else
    hipLaunchKernelGGL(
        HIP_KERNEL_NAME(attn_fwd_interval_kernel<DROP, 64>), grid,
        dim3(256), 0, stream, FWD_INTERVAL_ARGS);
#undef FWD_INTERVAL_ARGS
}

template <bool DROP>
void launch_bwd_interval(const void* q, const void* k, const void* v,
                         const void* out, const void* dout,
                         const float* lse, float* delta_ws, void* dq,
                         void* dk, void* dv, int64_t batch_heads,
                         int64_t seq, float scale, int64_t heads,
                         int64_t kv_heads, int64_t head_dim,
                         const int64_t* in_strides,
                         const int64_t* kv_strides,
                         const int64_t* o_strides,
                         const int64_t* do_strides,
                         const int64_t* g_strides,
                         const int64_t* gkv_strides, const int* seqlens,
                         const int* kv_lo, const int* kv_hi,
                         const int* q_lo, const int* q_hi,
                         int64_t bound_sb, IntervalDrop<DROP> da,
                         hipStream_t stream) {
  // dV over the B * Hkv grid -> dQ over the group-aware grid (publishes
  // delta per query head) -> dK
  const int64_t group = heads / kv_heads;
  const int64_t bhkv = batch_heads / group;
  const unsigned n = (unsigned)((seq + 127) / 128);
  const dim3 kvgrid(n, (unsigned)bhkv);
  const dim3 qgrid(n * (unsigned)group, (unsigned)bhkv);
#define KV_INTERVAL_ARGS(res)                                            \
  reinterpret_cast<const short*>(q), reinterpret_cast<const short*>(k),  \
    reinterpret_cast<const short*>(v),                                 \
    reinterpret_cast<const short*>(dout), lse, delta_ws,               \
    reinterpret_cast<short*>(res), seq, scale, heads, group,           \
    in_strides[0], in_strides[1], in_strides[2], kv_strides[0],        \
    kv_strides[1], kv_strides[2], do_strides[0], do_strides[1],        \
    do_strides[2], gkv_strides[0], gkv_strides[1], gkv_strides[2],     \
    seqlens, q_lo, q_hi, bound_sb, da
  auto launch = [&](auto d_c) {
    constexpr int D = decltype(d_c)::value;
    hipLaunchKernelGGL(
        HIP_KERNEL_NAME(attn_bwd_kv_interval_kernel<DROP, false, D>),
        kvgrid, dim3(256), 0, stream, KV_INTERVAL_ARGS(dv));
    hipLaunchKernelGGL(
        HIP_KERNEL_NAME(attn_bwd_dq_interval_kernel<DROP, D>), qgrid,
        dim3(256), 0, stream, reinterpret_cast<const short*>(q),
        reinterpret_cast<const short*>(k),
        reinterpret_cast<const short*>(v),
        reinterpret_cast<const short*>(dout), lse, delta_ws,
        reinterpret_cast<short*>(dq), reinterpret_cast<const short*>(out),
        seq, scale, heads, group, in_strides[0], in_strides[1],
        in_strides[2], kv_strides[0], kv_strides[1], kv_strides[2],
        do_strides[0], do_strides[1], do_strides[2], g_strides[0],
        g_strides[1], g_strides[2], o_strides[0], o_strides[1],
        o_strides[2], seqlens, kv_lo, kv_hi, bound_sb, da);
    hipLaunchKernelGGL(
        HIP_KERNEL_NAME(attn_bwd_kv_interval_kernel<DROP, true, D>),
        kvgrid, dim3(256), 0, stream, KV_INTERVAL_ARGS(dk));
  };
  if (head_dim == 128)
    launch(std::integral_constant<int, 128>{});
  else
    launch(std::integral_constant<int, 64>{});
#undef KV_INTERVAL_ARGS
}

}  // namespace
