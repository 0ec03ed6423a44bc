// Hand-written CDNA4 (gfx950) flash attention, head_dim 64 and 128,
// bf16, causal or not, optional in-kernel dropout, optional per-sample
// lengths for right-padded batches (sample_len below).
//
// Replaces the AOTriton SDPA kernels on the BERT/GPT hot path (BERT-Large
// shape b128 s512 h16 d64 on MI355X: bwd ~1190 us for the three kernels,
// profiles/attn_bwd_tiles_ab.txt; fwd profiles/attn_fwd_lean_ab.txt).
//
// Forward structure (one 32-row q-block per wave, 64-key kv tiles taken
// as two 32-key sub-tiles):
//  * swapped QK^T: S^T = K @ Q^T via v_mfma_f32_32x32x16_bf16, so each
//    lane owns ONE q-row's scores (16 kv values per lane, the partner
//    lane l^32 holds the other 16) -> the row max is 8 v_max3 + one
//    v_permlane32_swap exchange, no LDS.
//  * the running max is kept on the RAW accumulator values and
//    P = exp2(fma(S, scale*log2e, -m*scale*log2e)): one fma per v_exp_f32.
//  * O accumulated TRANSPOSED: O^T = V^T @ P^T, so the online rescale by
//    alpha is a lane-local scalar multiply; it is DEFERRED: a wave-uniform
//    branch takes it only when a row max grew by more than 2^8, else the
//    stale max stays (P <= 2^8).  Row sums stay per-lane partials until
//    the epilogue.
//  * P^T fragments assembled in-register: pack f32 pairs to bf16 dwords
//    and exchange halves with v_permlane32_swap.
//  * K and V tiles are staged alike, 8 lanes per 128-byte row piece
//    (whole cache lines per load instruction); K is read back by rows
//    (ds_read_b128), V sits in the dual-use row image of
//    attn_lds_image.h and its V^T operands are ds_read_b64_tr_b16 reads.
//  * O is parked in the freed K buffers and stored as whole rows.
// Saves per-row LSE (m*scale + log l) for the backward.
//
// Backward: three kernels launched dV -> dQ -> dK (kv-parallel for dV
// and dK, q-parallel for dQ), each lane owning its output row — no
// atomics; d64 non-causal calls without dropout run dQ -> dK+dV instead,
// one kv-parallel kernel for both (attn_bwd_dkdv_kernel, same bits;
// split_dkdv / EPL_ATTN_BWD_SPLIT=1 keep the split pair).  The dQ kernel
// computes D_i = rowsum(dO*O) from the rows it already loads and
// publishes it for the dK kernel.  64-row q/dO (or
// K/V) chunks are staged in one LDS image per tile that is read by rows
// (ds_read_b128) for S and dP and by columns (ds_read_b64_tr_b16) for
// dV^T, dK^T and dQ; the dV/dK kernels stage the chunk's -lse/scale and
// -delta next to it and start the S and dP chains from them.
// EPL_ATTN_BWD_TILES=legacy selects the previous tile bodies (2-byte
// LDS gathers, row constants from global memory) for a same-process
// A/B.  All kernels take (batch, head, seq) strides so the qkv-unbind
// views are consumed without copies.
//
// Non-causal grids run in the XCD-local block order of
// attn_block_order.h: the 128-row blocks of a batch-head, which read the
// same operands, share one L2 instead of fetching them once per XCD.

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <type_traits>

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

DEVI unsigned short f2bf(float f) {
  union { float f; unsigned int i; } v;
  v.f = f;
  unsigned int lsb = (v.i >> 16) & 1u;
  return (unsigned short)((v.i + 0x7fffu + lsb) >> 16);
}

DEVI unsigned int pack2(float a, float b) {
  return (unsigned int)f2bf(a) | ((unsigned int)f2bf(b) << 16);
}

// C/D row for reg r, half hi of v_mfma_f32_32x32x16_bf16
DEVI int crow(int r, int hi) {
  return (r & 3) + 8 * (r >> 2) + 4 * hi;
}

// two floats -> packed bf16 pair, round-to-nearest-even, in one
// v_cvt_pk_bf16_f32 (bit-identical to pack2 for finite values)
DEVI unsigned int cvt_pk_bf16(float a, float b) {
  f32x2 f = {a, b};
  return __builtin_bit_cast(unsigned int,
                            __builtin_convertvector(f, bf16v2));
}

// assemble the P^T mfma operand from 8 f32 scores (p[0..7] at rows
// crow(0..7, hi)): returns bf16x8 with element j = P at kv = hi*8+j.
// HW selects the packed hardware convert; the legacy backward tiles keep
// the software rounding so the A/B switch compares the parent's bodies.
template <bool HW = false>
DEVI bf16x8 assemble_pfrag(const float* p) {
  unsigned int c0 = HW ? cvt_pk_bf16(p[0], p[1]) : pack2(p[0], p[1]);
  unsigned int c1 = HW ? cvt_pk_bf16(p[2], p[3]) : pack2(p[2], p[3]);
  unsigned int c2 = HW ? cvt_pk_bf16(p[4], p[5]) : pack2(p[4], p[5]);
  unsigned int c3 = HW ? cvt_pk_bf16(p[6], p[7]) : pack2(p[6], p[7]);
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
// new tile bodies and of the forward's V tile: layout and fragment
// readers in attn_lds_image.h
using attn_img::img_off;
using attn_img::img_pitch;
using attn_img::tr_frag;

// staging-store address of columns col..col+7 (col % 8 == 0) of a row:
// the legacy tiles' padded rows, or the dual-use image of the new ones
template <bool TR, int D>
DEVI short* img_at(short (&img)[64][TR ? img_pitch<D>() : D + 8], int row,
                   int col) {
  return TR ? &img[0][0] + img_off<D>(row, col >> 3) : &img[row][col];
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

// MASKED tiles: the legacy test (qg >= seq || (causal && mykv > qg) ||
// mykv >= seq) for tile row c = crow(r, hi), qg = q0 + c, as two 32-bit
// bounds: masked <=> c < lo || c >= hi_
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

// ============================================================================
// forward (v4): KVBLK = 64; K (padded row copies, conflict-free
// ds_read_b128 fragments) and V (row image, transposed reads) staged in
// LDS once per block per tile.  Measured: explicit double-buffering and
// register prefetch both REGRESS (hipcc schedules the simple form best
// at 3-4 waves/SIMD) - keep this structure.  One softmax step per 64-key
// tile (both S sub-tiles first) measured the same as two 32-key steps and
// spills the d64 dropout kernel (profiles/attn_fwd_lean_ab.txt).
//
// v3: the kv loop is SPLIT into a branch-free bulk phase (tiles that are
// provably full: no seq-bound or causal masking, no per-wave break — the
// compiler pipelines it like the non-causal fast path) and a masked
// phase covering the causal diagonal (<= 2 tiles) and the seq tail.
// Round-1 measurement showed the single masked loop ran EVERY causal
// tile 33-46% slower per tile than the non-causal loop ran the same
// machine code — the masking ALU + dynamic break cost lands on all
// tiles, not just diagonal ones.
// ============================================================================

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
  bf16x8 pf0 = assemble_pfrag<true>(&s[0]);
  bf16x8 pf1 = assemble_pfrag<true>(&s[8]);
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

template <bool DROP, int D>
__global__ __launch_bounds__(256, D == 64 ? 3 : 2) void attn_fwd_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, short* __restrict__ out,
    float* __restrict__ lse, int64_t seq, float scale, int causal,
    int64_t heads, int64_t in_sb, int64_t in_sh, int64_t in_ss,
    int64_t o_sb, int64_t o_sh, int64_t o_ss,
    unsigned int* __restrict__ mask, int64_t mask_w,
    unsigned long long seed, int drop_thresh, float inv_keep,
    const int* __restrict__ seqlens) {
  // V: [kv][d] row image (attn_lds_image.h), read transposed for PV
  __shared__ __attribute__((aligned(16))) short
      ldsV[2][64 * img_pitch<D>()];
  // K: [kv][d] padded rows; after the loop, the block's 128 O rows
  __shared__ __attribute__((aligned(16))) short ldsK[2][64][D + 8];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int hi = lane >> 5;
  const int lq = lane & 31;
  // causal: qb rides the Y axis with bh on X — dispatch is x-fastest,
  // so EVERY batch-head of the longest q-block launches before the
  // next-longest (global longest-first packing).  The old per-row
  // reversal still launched one longest block in the LAST row — a
  // ~1-block drain tail that left causal at ~35% packing efficiency
  // at s4096 (profiles/r02_attention_ab.txt wave-residency probe).
  // non-causal: the XCD-local order of attn_block_order.h, so that the
  // q-blocks of a batch-head stream its K and V through one L2
  const BlockPos pos = block_pos(causal, true);
  const int64_t bh = pos.bh;
  const int64_t boff = (bh / heads) * in_sb + (bh % heads) * in_sh;
  const int64_t q0_blk = pos.blk * 128;
  const int64_t q0 = q0_blk + wave * 32;
  const int64_t len = sample_len(seqlens, bh / heads, seq);
  const int64_t myq = q0 + lq;
  // padded rows are written as zeros here, ahead of the loop, so that
  // past this point seq is a pitch only and the loop holds the same
  // scalars as before (len in the place of seq)
  if (myq >= len && myq < seq) {
    zero_row<D>(out + (bh / heads) * o_sb + (bh % heads) * o_sh +
                    myq * o_ss, hi);
    if (hi == 0) lse[bh * seq + myq] = 0.f;
  }
  // a block wholly inside the padding (an empty sample included) loads
  // nothing and leaves before any barrier
  if (q0_blk >= len) return;
  const bool active = q0 < len;
  const short* qp = q + boff;
  const short* kp = k + boff;
  const short* vp = v + boff;

  const int64_t qrow = myq < len ? myq : len - 1;

  bf16x8 qfrag[D / 16];
#pragma unroll
  for (int c = 0; c < D / 16; ++c)
    qfrag[c] = *reinterpret_cast<const bf16x8*>(
        qp + qrow * in_ss + hi * 8 + 16 * c);

  f32x16 ot[D / 32] = {};
  // m: running RAW row maximum; l: this lane's partial row sum (fwd_tile)
  float m = -1e30f, l = 0.f;
  const float c2 = scale * 1.44269504088896341f;

  // bulk tiles are provably full for EVERY lane of the block: below the
  // causal diagonal (kv < q0_blk <= myq) and inside the length
  const int64_t len64 = len & ~(int64_t)63;
  const int64_t bulk_end = causal ? (q0_blk < len64 ? q0_blk : len64) : len64;
  const int64_t blk_kv_end =
      causal ? (q0_blk + 128 < len ? q0_blk + 128 : len) : len;

  // Single-barrier double-buffered staging: the NEXT tile's global
  // loads issue right after the barrier and their latency hides under
  // the CURRENT tile's MFMA/softmax; the ds_write that consumes them
  // (start of the next iteration) is where the vmcnt wait lands.  One
  // __syncthreads per 64-kv tile instead of two (PMC r2: 38% of
  // wave-cycles were parked at barriers).
  // Eight consecutive lanes fetch one 128-byte piece of a row, so a wave
  // instruction covers 8 whole cache lines (a lane per row touched 64)
  // and lands as one conflict-free ds_write_b128 per 8 lanes; K and V
  // are staged alike.
  const int stage_row = threadIdx.x >> 3;        // 0..31, +32 per half
  const int stage_seg = (threadIdx.x & 7) * 8;   // +64 per 128-byte piece
  bf16x8 pv[2][D / 64], pk[2][D / 64];
  auto load_tile = [&](int64_t kv0) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      int64_t vrow = kv0 + stage_row + half * 32;
      if (vrow >= len) vrow = len - 1;   // masked columns never contribute
#pragma unroll
      for (int s = 0; s < D / 64; ++s) {
        const int col = stage_seg + s * 64;
        pv[half][s] =
            *reinterpret_cast<const bf16x8*>(vp + vrow * in_ss + col);
        pk[half][s] =
            *reinterpret_cast<const bf16x8*>(kp + vrow * in_ss + col);
      }
    }
  };
  auto write_tile = [&](int b) {
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int s = 0; s < D / 64; ++s) {
        const int row = stage_row + half * 32;
        const int col = stage_seg + s * 64;
        *reinterpret_cast<bf16x8*>(
            &ldsV[b][img_off<D>(row, col >> 3)]) = pv[half][s];
        *reinterpret_cast<bf16x8*>(&ldsK[b][row][col]) = pk[half][s];
      }
  };

  unsigned int* maskrow =
      DROP ? mask + bh * seq * mask_w : (unsigned int*)nullptr;
  const unsigned int seed0 = (unsigned int)seed;
  const unsigned int seed1 = (unsigned int)(seed >> 32);
  const unsigned int bh32 = (unsigned int)bh;

  int buf = 0;
  if (blk_kv_end > 0) load_tile(0);
  int64_t kv0 = 0;
  for (; kv0 < bulk_end; kv0 += 64) {
    write_tile(buf);
    __syncthreads();
    if (kv0 + 64 < blk_kv_end) load_tile(kv0 + 64);
#pragma unroll
    for (int sub = 0; sub < 64; sub += 32)
      fwd_tile<false, DROP, D>(ldsK[buf], ldsV[buf], sub, kv0 + sub, len,
                               myq, c2, causal, qfrag, ot, m, l, lq, hi,
                               maskrow, mask_w, seed0, seed1, bh32,
                               drop_thresh, inv_keep);
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
        fwd_tile<true, DROP, D>(ldsK[buf], ldsV[buf], sub, kvs, len, myq,
                                c2, causal, qfrag, ot, m, l, lq, hi,
                                maskrow, mask_w, seed0, seed1, bh32,
                                drop_thresh, inv_keep);
      }
    }
    buf ^= 1;
  }

  // the two lanes of a row applied the same alpha throughout, so their
  // partial sums add exactly.  No wave has diverged or left since the
  // loop: EXEC is all ones for the swap.
  {
    unsigned int a, b;
    both_halves(__builtin_bit_cast(unsigned int, l), a, b);
    l = __builtin_bit_cast(float, a) + __builtin_bit_cast(float, b);
  }
  const float inv_l = 1.f / l;
  short* ob = out + (bh / heads) * o_sb + (bh % heads) * o_sh;
  // O leaves through the K buffers, now free: each lane parks its row
  // (8-byte pieces), then eight (d128: sixteen) lanes store one whole row
  // as 16-byte pieces.  A lane per row wrote 8 bytes to each of 32 lines
  // per instruction.  Waves past len park garbage and store nothing;
  // every wave of the block reaches both barriers.
  short* ldsO = &ldsK[0][0][0] + wave * 32 * (D + 8);
  __syncthreads();              // every wave is done with the last K tile
#pragma unroll
  for (int j = 0; j < D / 32; ++j)
    store_acc_bf16(ldsO + lq * (D + 8) + j * 32, ot[j] * inv_l, hi);
  __syncthreads();
  constexpr int LPR = D / 8;    // lanes per row
#pragma unroll
  for (int r0 = 0; r0 < 32; r0 += 64 / LPR) {
    const int r = r0 + lane / LPR;
    const int col = (lane % LPR) * 8;
    const bf16x8 piece =
        *reinterpret_cast<const bf16x8*>(ldsO + r * (D + 8) + col);
    if (q0 + r < len)
      *reinterpret_cast<bf16x8*>(ob + (q0 + r) * o_ss + col) = piece;
  }
  // m is a raw maximum; lse is in score units
  if (hi == 0 && myq < len) lse[bh * seq + myq] = m * scale + __logf(l);
}

// ============================================================================
// backward kernels A (kv-parallel): dV-only and dK-only, one wave per
// 32-key kv tile, looping 64-row q/dO chunks staged in LDS; half the
// accumulators of the combined dK+dV kernel further down each -> 3
// waves/SIMD instead of 2.  The q loop runs in three phases: masked
// causal-diagonal tiles, branch-free bulk tiles, masked seq tail (same
// rationale as the forward v3 split).
// ============================================================================

// one 32-row q sub-tile (of the 64-row staged chunk) of the dV
// accumulation; `sub` selects the LDS half.  DROP: dV = P_d^T dO, so P
// is masked+rescaled with the forward's keep bits (bit mykv&31 of the
// mask word of row qg — one broadcast word load per row).
template <bool MASKED, bool DROP, int D>
DEVI void dv_tile(const short (&ldsQ)[64][D + 8],
                  const short (&ldsDO)[64][D + 8],
                  int sub, int64_t q0, int64_t seq, int64_t mykv,
                  float scale, int causal, const float* lsep,
                  const bf16x8 (&kfrag)[D / 16], f32x16 (&dvt)[D / 32],
                  int lkv, int hi, const unsigned int* maskrow,
                  int64_t mask_w, float inv_keep) {
  f32x16 st = {};
#pragma unroll
  for (int c = 0; c < D / 16; ++c) {
    bf16x8 qf = *reinterpret_cast<const bf16x8*>(
        &ldsQ[sub + lkv][hi * 8 + 16 * c]);
    st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf, kfrag[c], st, 0, 0, 0);
  }
  float p[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t qg = q0 + crow(r, hi);
    const int64_t qgc = qg < seq ? qg : seq - 1;
    if (MASKED) {
      bool masked = qg >= seq || (causal && mykv > qg) || mykv >= seq;
      p[r] = masked ? 0.f : __expf(st[r] * scale - lsep[qgc]);
    } else {
      p[r] = __expf(st[r] * scale - lsep[qg]);
    }
    if (DROP) {
      const int64_t kvc = mykv < seq ? mykv : seq - 1;
      const unsigned int w = maskrow[qgc * mask_w + (kvc >> 5)];
      p[r] *= ((w >> (kvc & 31)) & 1u) ? inv_keep : 0.f;
    }
  }
  bf16x8 pb0 = assemble_pfrag(&p[0]);
  bf16x8 pb1 = assemble_pfrag(&p[8]);
#pragma unroll
  for (int qc = 0; qc < 2; ++qc) {
    bf16x8 pb = qc == 0 ? pb0 : pb1;
#pragma unroll
    for (int dj = 0; dj < D / 32; ++dj) {
      bf16x8 dot;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int qr = sub + qc * 16 + hi * 8 + j;
        dot[j] = ldsDO[qr][dj * 32 + lkv];
      }
      dvt[dj] =
          __builtin_amdgcn_mfma_f32_32x32x16_bf16(dot, pb, dvt[dj], 0, 0, 0);
    }
  }
}

// one 32-row q sub-tile of the dK accumulation.  DROP mirrors dq_tile:
// P undropped, the dO.V term masked+rescaled.
template <bool MASKED, bool DROP, int D>
DEVI void dk_tile(const short (&ldsQ)[64][D + 8],
                  const short (&ldsDO)[64][D + 8],
                  int sub, int64_t q0, int64_t seq, int64_t mykv,
                  float scale, int causal, const float* lsep,
                  const float* dltp, const bf16x8 (&kfrag)[D / 16],
                  const bf16x8 (&vfrag)[D / 16], f32x16 (&dkt)[D / 32],
                  int lkv, int hi, const unsigned int* maskrow,
                  int64_t mask_w, float inv_keep) {
  f32x16 st = {};
  f32x16 dpt = {};
#pragma unroll
  for (int c = 0; c < D / 16; ++c) {
    bf16x8 qf = *reinterpret_cast<const bf16x8*>(
        &ldsQ[sub + lkv][hi * 8 + 16 * c]);
    bf16x8 dof = *reinterpret_cast<const bf16x8*>(
        &ldsDO[sub + lkv][hi * 8 + 16 * c]);
    st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf, kfrag[c], st, 0, 0, 0);
    dpt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dof, vfrag[c], dpt, 0, 0,
                                                  0);
  }
  float ds[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t qg = q0 + crow(r, hi);
    const int64_t qgc = qg < seq ? qg : seq - 1;
    float dp = dpt[r];
    if (DROP) {
      const int64_t kvc = mykv < seq ? mykv : seq - 1;
      const unsigned int w = maskrow[qgc * mask_w + (kvc >> 5)];
      dp *= ((w >> (kvc & 31)) & 1u) ? inv_keep : 0.f;
    }
    if (MASKED) {
      bool masked = qg >= seq || (causal && mykv > qg) || mykv >= seq;
      float pv = masked ? 0.f : __expf(st[r] * scale - lsep[qgc]);
      ds[r] = masked ? 0.f : pv * (dp - dltp[qgc]) * scale;
    } else {
      float pv = __expf(st[r] * scale - lsep[qg]);
      ds[r] = pv * (dp - dltp[qg]) * scale;
    }
  }
  bf16x8 db0 = assemble_pfrag(&ds[0]);
  bf16x8 db1 = assemble_pfrag(&ds[8]);
#pragma unroll
  for (int qc = 0; qc < 2; ++qc) {
    bf16x8 db = qc == 0 ? db0 : db1;
#pragma unroll
    for (int dj = 0; dj < D / 32; ++dj) {
      bf16x8 qt;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int qr = sub + qc * 16 + hi * 8 + j;
        qt[j] = ldsQ[qr][dj * 32 + lkv];
      }
      dkt[dj] =
          __builtin_amdgcn_mfma_f32_32x32x16_bf16(qt, db, dkt[dj], 0, 0, 0);
    }
  }
}

// ----------------------------------------------------------------------------
// New tile bodies (default; EPL_ATTN_BWD_TILES=legacy selects the ones
// above).  Same products; what changes is how the operands arrive:
//  * Q/dO live in the dual-use image (img_off) and the transposed
//    fragments come from two ds_read_b64_tr_b16 instead of eight 2-byte
//    reads;
//  * lse (and delta) of the chunk's 64 rows are staged in LDS with the
//    chunk and read as four ds_read_b128 instead of 16 global loads;
//  * bf16 rounding is v_cvt_pk_bf16_f32.
// lseL/dltL point at the 32 row constants of this sub-tile, staged as
// -lse/scale and -delta so the S and dP chains start from them and
// P = exp2(scale*log2(e) * S') needs no subtraction; rows past seq hold
// the clamped row's value, as the legacy bodies read it.
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
  bf16x8 pb0 = assemble_pfrag<true>(&p[0]);
  bf16x8 pb1 = assemble_pfrag<true>(&p[8]);
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
  bf16x8 db0 = assemble_pfrag<true>(&ds[0]);
  bf16x8 db1 = assemble_pfrag<true>(&ds[8]);
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

template <bool DROP, bool DBUF, int D, bool TR>
__global__ __launch_bounds__(256, D == 64 ? (DBUF ? 3 : 4)
                                          : (TR && !DROP ? 3 : 2))
void attn_bwd_dv_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ dout, const float* __restrict__ lse,
    short* __restrict__ dv, int64_t seq, float scale, int causal,
    int64_t heads, int64_t in_sb, int64_t in_sh, int64_t in_ss,
    int64_t do_sb, int64_t do_sh, int64_t do_ss, int64_t g_sb,
    int64_t g_sh, int64_t g_ss,
    const unsigned int* __restrict__ mask, int64_t mask_w,
    float inv_keep, const int* __restrict__ seqlens) {
  // TR: dual-use image + the chunk's 64 -lse/scale values
  constexpr int PITCH = TR ? img_pitch<D>() : D + 8;
  __shared__ __attribute__((aligned(16))) short
      ldsQ[DBUF ? 2 : 1][64][PITCH];
  __shared__ __attribute__((aligned(16))) short
      ldsDO[DBUF ? 2 : 1][64][PITCH];
  __shared__ __attribute__((aligned(16))) float ldsL[DBUF ? 2 : 1][64];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int hi = lane >> 5;
  const int lkv = lane & 31;
  // causal: kv0 rides the Y axis (ascending = longest q-range first),
  // bh on X — global longest-first packing like the fwd kernel;
  // non-causal: XCD-local order, the kv-blocks of a batch-head stream its
  // Q and dO through one L2
  const BlockPos pos = block_pos(causal, false);
  const int64_t bh = pos.bh;
  const int64_t kv0_blk = pos.blk * 128;
  const int64_t kv0 = kv0_blk + wave * 32;
  const int64_t len = sample_len(seqlens, bh / heads, seq);
  const int64_t mykv = kv0 + lkv;
  // padded key rows are zeroed ahead of the loop and a block wholly
  // inside the padding loads nothing (see attn_fwd_kernel)
  if (mykv >= len && mykv < seq)
    zero_row<D>(dv + (bh / heads) * g_sb + (bh % heads) * g_sh +
                    mykv * g_ss, hi);
  if (kv0_blk >= len) return;
  const bool active = kv0 < len;
  const int64_t boff = (bh / heads) * in_sb + (bh % heads) * in_sh;
  const short* qp = q + boff;
  const short* kp = k + boff;
  const short* dop = dout + (bh / heads) * do_sb + (bh % heads) * do_sh;
  const float* lsep = lse + bh * seq;

  const int64_t kvrow = mykv < len ? mykv : len - 1;
  bf16x8 kfrag[D / 16];
#pragma unroll
  for (int c = 0; c < D / 16; ++c)
    kfrag[c] = *reinterpret_cast<const bf16x8*>(
        kp + kvrow * in_ss + hi * 8 + 16 * c);

  f32x16 dvt[D / 32] = {};
  const int stage_row = threadIdx.x >> 3;
  const int stage_seg = (threadIdx.x & 7) * 8;

  // DBUF=false: stage 64 q rows straight to LDS per barrier pair.
  // DBUF=true: software pipeline — this chunk's rows were prefetched
  // into registers during the previous chunk's MFMAs; commit them to
  // the alternate LDS buffer, one barrier, then issue the next chunk's
  // global loads so they hide under this chunk's compute (the fwd v7
  // staging pattern applied to the q/dO loop).
  bf16x8 rq[2][D / 64], rdo[2][D / 64];
  float rl = 0.f;   // TR: wave 0 carries the chunk's -lse/scale values
  const float neg_inv_scale = -1.f / scale;
  auto prefetch = [&](int64_t q0) {
    if (TR && wave == 0) {
      const int64_t qr = q0 + lane;
      rl = lsep[qr < len ? qr : len - 1] * neg_inv_scale;
    }
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
    if (TR && wave == 0) ldsL[buf][lane] = rl;
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int s = 0; s < D / 64; ++s) {
        *reinterpret_cast<bf16x8*>(
            img_at<TR, D>(ldsQ[buf], stage_row + half * 32,
                          stage_seg + s * 64)) =
            rq[half][s];
        *reinterpret_cast<bf16x8*>(
            img_at<TR, D>(ldsDO[buf], stage_row + half * 32,
                          stage_seg + s * 64)) =
            rdo[half][s];
      }
  };
  auto stage_q64 = [&](int64_t q0) {
    __syncthreads();
    if (TR && wave == 0) {
      const int64_t qr = q0 + lane;
      ldsL[0][lane] = lsep[qr < len ? qr : len - 1] * neg_inv_scale;
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      int64_t qr = q0 + stage_row + half * 32;
      if (qr >= len) qr = len - 1;
#pragma unroll
      for (int seg = 0; seg < D; seg += 64) {
        *reinterpret_cast<bf16x8*>(
            img_at<TR, D>(ldsQ[0], stage_row + half * 32,
                          stage_seg + seg)) =
            *reinterpret_cast<const bf16x8*>(
                qp + qr * in_ss + stage_seg + seg);
        *reinterpret_cast<bf16x8*>(
            img_at<TR, D>(ldsDO[0], stage_row + half * 32,
                          stage_seg + seg)) =
            *reinterpret_cast<const bf16x8*>(
                dop + qr * do_ss + stage_seg + seg);
      }
    }
    __syncthreads();
  };

  const unsigned int* maskrow =
      DROP ? mask + bh * seq * mask_w : (const unsigned int*)nullptr;
  // one 32-row sub-tile from LDS buffer rb: new or legacy body
  auto tile = [&](auto masked, int rb, int sub, int64_t q0s) {
    constexpr bool M = decltype(masked)::value;
    if constexpr (TR)
      dv_tile_tr<M, DROP, D>(&ldsQ[rb][0][0], &ldsDO[rb][0][0],
                             &ldsL[rb][sub], sub, q0s, len, mykv, scale,
                             causal, kfrag, dvt, lkv, hi, maskrow, mask_w,
                             inv_keep);
    else
      dv_tile<M, DROP, D>(ldsQ[rb], ldsDO[rb], sub, q0s, len, mykv, scale,
                          causal, lsep, kfrag, dvt, lkv, hi, maskrow,
                          mask_w, inv_keep);
  };
  constexpr std::true_type MASKED_T{};
  constexpr std::false_type PLAIN_T{};

  // unified 64-row chunk loop; the phase test (masked causal diagonal /
  // branch-free bulk / masked seq tail) is block-uniform per chunk
  const int64_t diag_end =
      causal ? (kv0_blk + 128 < len ? kv0_blk + 128 : len) : 0;
  const int64_t bulk_end = len & ~(int64_t)63;
  if (!DBUF) {
    // two-barrier direct staging, phase-split loops (the measured r2
    // baseline — kept verbatim so the fallback stays spill-free)
    int64_t q0 = causal ? kv0_blk : 0;
    for (; q0 < diag_end; q0 += 64) {
      stage_q64(q0);
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
      stage_q64(q0);
#pragma unroll
      for (int sub = 0; sub < 64; sub += 32)
        tile(PLAIN_T, 0, sub, q0 + sub);
    }
    for (; q0 < len; q0 += 64) {
      stage_q64(q0);
      if (!active) continue;
#pragma unroll
      for (int sub = 0; sub < 64; sub += 32) {
        const int64_t q0s = q0 + sub;
        if (q0s >= len) break;
        tile(MASKED_T, 0, sub, q0s);
      }
    }
  } else {
    const int64_t q_begin = causal ? kv0_blk : 0;
    int buf = 0;
    prefetch(q_begin);
    for (int64_t q0 = q_begin; q0 < len; q0 += 64) {
      commit(buf);
      __syncthreads();
      if (q0 + 64 < len) prefetch(q0 + 64);
      const int rb = buf;
      buf ^= 1;
      const bool plain = q0 >= diag_end && q0 + 63 < bulk_end;
      if (plain) {
#pragma unroll
        for (int sub = 0; sub < 64; sub += 32)
          tile(PLAIN_T, rb, sub, q0 + sub);
      } else if (active) {
#pragma unroll
        for (int sub = 0; sub < 64; sub += 32) {
          const int64_t q0s = q0 + sub;
          if (q0s >= len) break;
          if (causal && q0s + 31 < kv0) continue;
          tile(MASKED_T, rb, sub, q0s);
        }
      }
    }
  }
  if (!active || mykv >= len) return;
  short* dvp = dv + (bh / heads) * g_sb + (bh % heads) * g_sh +
               mykv * g_ss;
#pragma unroll
  for (int dj = 0; dj < D / 32; ++dj) {
    if constexpr (TR) {
      store_acc_bf16(dvp + dj * 32, dvt[dj], hi);
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        dvp[dj * 32 + crow(r, hi)] = (short)f2bf(dvt[dj][r]);
    }
  }
}

template <bool DROP, bool DBUF, int D, bool TR>
__global__ __launch_bounds__(256, D == 64 ? 3 : 2) void attn_bwd_dk_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, const short* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    short* __restrict__ dk, int64_t seq, float scale, int causal,
    int64_t heads, int64_t in_sb, int64_t in_sh, int64_t in_ss,
    int64_t do_sb, int64_t do_sh, int64_t do_ss, int64_t g_sb,
    int64_t g_sh, int64_t g_ss,
    const unsigned int* __restrict__ mask, int64_t mask_w,
    float inv_keep, const int* __restrict__ seqlens) {
  constexpr int PITCH = TR ? img_pitch<D>() : D + 8;
  __shared__ __attribute__((aligned(16))) short
      ldsQ[DBUF ? 2 : 1][64][PITCH];
  __shared__ __attribute__((aligned(16))) short
      ldsDO[DBUF ? 2 : 1][64][PITCH];
  // TR: [0] = -lse/scale, [1] = -delta of the chunk's 64 rows
  __shared__ __attribute__((aligned(16))) float ldsL[DBUF ? 2 : 1][2][64];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int hi = lane >> 5;
  const int lkv = lane & 31;
  const BlockPos pos = block_pos(causal, false);   // see attn_bwd_dv_kernel
  const int64_t bh = pos.bh;
  const int64_t kv0_blk = pos.blk * 128;
  const int64_t kv0 = kv0_blk + wave * 32;
  const int64_t len = sample_len(seqlens, bh / heads, seq);
  const int64_t mykv = kv0 + lkv;
  // padded key rows are zeroed ahead of the loop and a block wholly
  // inside the padding loads nothing (see attn_fwd_kernel)
  if (mykv >= len && mykv < seq)
    zero_row<D>(dk + (bh / heads) * g_sb + (bh % heads) * g_sh +
                    mykv * g_ss, hi);
  if (kv0_blk >= len) return;
  const bool active = kv0 < len;
  const int64_t boff = (bh / heads) * in_sb + (bh % heads) * in_sh;
  const short* qp = q + boff;
  const short* kp = k + boff;
  const short* vp = v + boff;
  const short* dop = dout + (bh / heads) * do_sb + (bh % heads) * do_sh;
  const float* lsep = lse + bh * seq;
  const float* dltp = delta + bh * seq;

  const int64_t kvrow = mykv < len ? mykv : len - 1;
  bf16x8 kfrag[D / 16], vfrag[D / 16];
#pragma unroll
  for (int c = 0; c < D / 16; ++c) {
    kfrag[c] = *reinterpret_cast<const bf16x8*>(
        kp + kvrow * in_ss + hi * 8 + 16 * c);
    vfrag[c] = *reinterpret_cast<const bf16x8*>(
        vp + kvrow * in_ss + hi * 8 + 16 * c);
  }

  f32x16 dkt[D / 32] = {};
  const int stage_row = threadIdx.x >> 3;
  const int stage_seg = (threadIdx.x & 7) * 8;

  // staging: same DBUF pipeline as the dV kernel (see comment there)
  bf16x8 rq[2][D / 64], rdo[2][D / 64];
  float rl = 0.f;   // TR: wave 0 carries -lse/scale, wave 1 -delta
  const float neg_inv_scale = -1.f / scale;
  auto prefetch = [&](int64_t q0) {
    if (TR && wave < 2) {
      const int64_t qr = q0 + lane;
      rl = (wave == 0 ? lsep : dltp)[qr < len ? qr : len - 1] *
           (wave == 0 ? neg_inv_scale : -1.f);
    }
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
    if (TR && wave < 2) ldsL[buf][wave][lane] = rl;
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int s = 0; s < D / 64; ++s) {
        *reinterpret_cast<bf16x8*>(
            img_at<TR, D>(ldsQ[buf], stage_row + half * 32,
                          stage_seg + s * 64)) =
            rq[half][s];
        *reinterpret_cast<bf16x8*>(
            img_at<TR, D>(ldsDO[buf], stage_row + half * 32,
                          stage_seg + s * 64)) =
            rdo[half][s];
      }
  };
  auto stage_q64 = [&](int64_t q0) {
    __syncthreads();
    if (TR && wave < 2) {
      const int64_t qr = q0 + lane;
      ldsL[0][wave][lane] =
          (wave == 0 ? lsep : dltp)[qr < len ? qr : len - 1] *
          (wave == 0 ? neg_inv_scale : -1.f);
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      int64_t qr = q0 + stage_row + half * 32;
      if (qr >= len) qr = len - 1;
#pragma unroll
      for (int seg = 0; seg < D; seg += 64) {
        *reinterpret_cast<bf16x8*>(
            img_at<TR, D>(ldsQ[0], stage_row + half * 32,
                          stage_seg + seg)) =
            *reinterpret_cast<const bf16x8*>(
                qp + qr * in_ss + stage_seg + seg);
        *reinterpret_cast<bf16x8*>(
            img_at<TR, D>(ldsDO[0], stage_row + half * 32,
                          stage_seg + seg)) =
            *reinterpret_cast<const bf16x8*>(
                dop + qr * do_ss + stage_seg + seg);
      }
    }
    __syncthreads();
  };

  const unsigned int* maskrow =
      DROP ? mask + bh * seq * mask_w : (const unsigned int*)nullptr;
  // one 32-row sub-tile from LDS buffer rb: new or legacy body
  auto tile = [&](auto masked, int rb, int sub, int64_t q0s) {
    constexpr bool M = decltype(masked)::value;
    if constexpr (TR)
      dk_tile_tr<M, DROP, D>(&ldsQ[rb][0][0], &ldsDO[rb][0][0],
                             &ldsL[rb][0][sub], &ldsL[rb][1][sub], sub,
                             q0s, len, mykv, scale, causal, kfrag, vfrag,
                             dkt, lkv, hi, maskrow, mask_w, inv_keep);
    else
      dk_tile<M, DROP, D>(ldsQ[rb], ldsDO[rb], sub, q0s, len, mykv, scale,
                          causal, lsep, dltp, kfrag, vfrag, dkt, lkv, hi,
                          maskrow, mask_w, inv_keep);
  };
  constexpr std::true_type MASKED_T{};
  constexpr std::false_type PLAIN_T{};
  const int64_t diag_end =
      causal ? (kv0_blk + 128 < len ? kv0_blk + 128 : len) : 0;
  const int64_t bulk_end = len & ~(int64_t)63;
  if (!DBUF) {
    int64_t q0 = causal ? kv0_blk : 0;
    for (; q0 < diag_end; q0 += 64) {
      stage_q64(q0);
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
      stage_q64(q0);
#pragma unroll
      for (int sub = 0; sub < 64; sub += 32)
        tile(PLAIN_T, 0, sub, q0 + sub);
    }
    for (; q0 < len; q0 += 64) {
      stage_q64(q0);
      if (!active) continue;
#pragma unroll
      for (int sub = 0; sub < 64; sub += 32) {
        const int64_t q0s = q0 + sub;
        if (q0s >= len) break;
        tile(MASKED_T, 0, sub, q0s);
      }
    }
  } else {
    const int64_t q_begin = causal ? kv0_blk : 0;
    int buf = 0;
    prefetch(q_begin);
    for (int64_t q0 = q_begin; q0 < len; q0 += 64) {
      commit(buf);
      __syncthreads();
      if (q0 + 64 < len) prefetch(q0 + 64);
      const int rb = buf;
      buf ^= 1;
      const bool plain = q0 >= diag_end && q0 + 63 < bulk_end;
      if (plain) {
#pragma unroll
        for (int sub = 0; sub < 64; sub += 32)
          tile(PLAIN_T, rb, sub, q0 + sub);
      } else if (active) {
#pragma unroll
        for (int sub = 0; sub < 64; sub += 32) {
          const int64_t q0s = q0 + sub;
          if (q0s >= len) break;
          if (causal && q0s + 31 < kv0) continue;
          tile(MASKED_T, rb, sub, q0s);
        }
      }
    }
  }
  if (!active || mykv >= len) return;
  short* dkp = dk + (bh / heads) * g_sb + (bh % heads) * g_sh +
               mykv * g_ss;
#pragma unroll
  for (int dj = 0; dj < D / 32; ++dj) {
    if constexpr (TR) {
      store_acc_bf16(dkp + dj * 32, dkt[dj], hi);
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        dkp[dj * 32 + crow(r, hi)] = (short)f2bf(dkt[dj][r]);
    }
  }
}

// ============================================================================
// combined dK+dV kernel (d64, non-causal, no dropout): dv_tile_tr and
// dk_tile_tr on one staged chunk.  Both split tiles compute
// S' = Q K^T - lse/scale from the same image and take the same 16 exp2;
// here the tile does that once and the block streams Q and dO once:
// 16 MFMA per 32x32 tile instead of 8 + 12.  K and V fragments and both
// accumulator pairs stay in registers, so the kernel runs at 2
// waves/SIMD.  delta comes from the dQ kernel's workspace: launch order
// dQ -> dK+dV.
//
// Every chain runs in the split tiles' order — S' and dP' from the row
// constants over c = 0..3, P = exp2(c2 S'), dV^T += dO^T P over (qc, dj),
// dS = P dP' scale in dk_tile_tr's expression, dK^T += Q^T dS over
// (qc, dj), chunks and sub-tiles ascending — so dk and dv carry the bits
// of attn_bwd_dv_kernel / attn_bwd_dk_kernel
// (tests/test_attention_dkdv_fused_gpu.py).
// ============================================================================
template <bool MASKED>
DEVI void dkdv_tile_tr(const short* imgQ, const short* imgDO,
                       const float* lseL, const float* dltL, int sub,
                       int64_t q0, int64_t seq, int64_t mykv, float scale,
                       const bf16x8 (&kfrag)[4], const bf16x8 (&vfrag)[4],
                       f32x16 (&dvt)[2], f32x16 (&dkt)[2], int lkv, int hi) {
  constexpr int D = 64;
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
  const RowMask rm(q0, seq, mykv, 0);
  float p[16], ds[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float e = __builtin_amdgcn_exp2f(st[r] * c2);
    if (MASKED) {
      const bool m = rm.masked(crow(r, hi));
      p[r] = m ? 0.f : e;
      ds[r] = m ? 0.f : e * dpt[r] * scale;
    } else {
      p[r] = e;
      ds[r] = e * dpt[r] * scale;
    }
  }
  const int lane = hi * 32 + lkv;
  bf16x8 pb0 = assemble_pfrag<true>(&p[0]);
  bf16x8 pb1 = assemble_pfrag<true>(&p[8]);
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
  bf16x8 db0 = assemble_pfrag<true>(&ds[0]);
  bf16x8 db1 = assemble_pfrag<true>(&ds[8]);
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

__global__ __launch_bounds__(256, 2) void attn_bwd_dkdv_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, const short* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    short* __restrict__ dk, short* __restrict__ dv, int64_t seq,
    float scale, int64_t heads, int64_t in_sb, int64_t in_sh,
    int64_t in_ss, int64_t do_sb, int64_t do_sh, int64_t do_ss,
    int64_t g_sb, int64_t g_sh, int64_t g_ss,
    const int* __restrict__ seqlens) {
  constexpr int D = 64;
  __shared__ __attribute__((aligned(16))) short ldsQ[2][64][img_pitch<D>()];
  __shared__ __attribute__((aligned(16))) short ldsDO[2][64][img_pitch<D>()];
  // [0] = -lse/scale, [1] = -delta of the chunk's 64 rows
  __shared__ __attribute__((aligned(16))) float ldsL[2][2][64];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int hi = lane >> 5;
  const int lkv = lane & 31;
  const BlockPos pos = block_pos(0, false);   // see attn_bwd_dv_kernel
  const int64_t bh = pos.bh;
  const int64_t kv0_blk = pos.blk * 128;
  const int64_t kv0 = kv0_blk + wave * 32;
  const int64_t len = sample_len(seqlens, bh / heads, seq);
  const int64_t mykv = kv0 + lkv;
  const int64_t goff = (bh / heads) * g_sb + (bh % heads) * g_sh +
                       mykv * g_ss;
  // padded key rows are zeroed ahead of the loop and a block wholly
  // inside the padding loads nothing (see attn_fwd_kernel)
  if (mykv >= len && mykv < seq) {
    zero_row<D>(dk + goff, hi);
    zero_row<D>(dv + goff, hi);
  }
  if (kv0_blk >= len) return;
  const bool active = kv0 < len;
  const int64_t boff = (bh / heads) * in_sb + (bh % heads) * in_sh;
  const short* qp = q + boff;
  const short* kp = k + boff;
  const short* vp = v + boff;
  const short* dop = dout + (bh / heads) * do_sb + (bh % heads) * do_sh;
  const float* lsep = lse + bh * seq;
  const float* dltp = delta + bh * seq;

  const int64_t kvrow = mykv < len ? mykv : len - 1;
  bf16x8 kfrag[D / 16], vfrag[D / 16];
#pragma unroll
  for (int c = 0; c < D / 16; ++c) {
    kfrag[c] = *reinterpret_cast<const bf16x8*>(
        kp + kvrow * in_ss + hi * 8 + 16 * c);
    vfrag[c] = *reinterpret_cast<const bf16x8*>(
        vp + kvrow * in_ss + hi * 8 + 16 * c);
  }

  f32x16 dvt[D / 32] = {};
  f32x16 dkt[D / 32] = {};
  const int stage_row = threadIdx.x >> 3;
  const int stage_seg = (threadIdx.x & 7) * 8;

  // the dV kernel's register-double-buffered single-barrier staging,
  // carrying the dK kernel's two row constants (wave 0 -lse/scale,
  // wave 1 -delta)
  bf16x8 rq[2], rdo[2];
  float rl = 0.f;
  const float neg_inv_scale = -1.f / scale;
  auto prefetch = [&](int64_t q0) {
    if (wave < 2) {
      const int64_t qr = q0 + lane;
      rl = (wave == 0 ? lsep : dltp)[qr < len ? qr : len - 1] *
           (wave == 0 ? neg_inv_scale : -1.f);
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      int64_t qr = q0 + stage_row + half * 32;
      if (qr >= len) qr = len - 1;
      rq[half] = *reinterpret_cast<const bf16x8*>(qp + qr * in_ss +
                                                  stage_seg);
      rdo[half] = *reinterpret_cast<const bf16x8*>(dop + qr * do_ss +
                                                   stage_seg);
    }
  };
  auto commit = [&](int buf) {
    if (wave < 2) ldsL[buf][wave][lane] = rl;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int o = img_off<D>(stage_row + half * 32, stage_seg >> 3);
      *reinterpret_cast<bf16x8*>(&ldsQ[buf][0][0] + o) = rq[half];
      *reinterpret_cast<bf16x8*>(&ldsDO[buf][0][0] + o) = rdo[half];
    }
  };

  const int64_t bulk_end = len & ~(int64_t)63;
  int buf = 0;
  prefetch(0);
  for (int64_t q0 = 0; q0 < len; q0 += 64) {
    commit(buf);
    __syncthreads();
    if (q0 + 64 < len) prefetch(q0 + 64);
    const int rb = buf;
    buf ^= 1;
    const short* imgQ = &ldsQ[rb][0][0];
    const short* imgDO = &ldsDO[rb][0][0];
    if (q0 + 63 < bulk_end) {
#pragma unroll
      for (int sub = 0; sub < 64; sub += 32)
        dkdv_tile_tr<false>(imgQ, imgDO, &ldsL[rb][0][sub],
                            &ldsL[rb][1][sub], sub, q0 + sub, len, mykv,
                            scale, kfrag, vfrag, dvt, dkt, lkv, hi);
    } else if (active) {
#pragma unroll
      for (int sub = 0; sub < 64; sub += 32) {
        const int64_t q0s = q0 + sub;
        if (q0s >= len) break;
        dkdv_tile_tr<true>(imgQ, imgDO, &ldsL[rb][0][sub],
                           &ldsL[rb][1][sub], sub, q0s, len, mykv, scale,
                           kfrag, vfrag, dvt, dkt, lkv, hi);
      }
    }
  }
  if (!active || mykv >= len) return;
#pragma unroll
  for (int dj = 0; dj < D / 32; ++dj) {
    store_acc_bf16(dv + goff + dj * 32, dvt[dj], hi);
    store_acc_bf16(dk + goff + dj * 32, dkt[dj], hi);
  }
}

// ============================================================================
// backward kernel B (q-parallel): dQ.  K and V tiles staged in LDS as
// row copies per block; row fragments via ds_read_b128, K-transposed
// fragments via 2-byte LDS reads.  Like the forward, the kv loop is
// split into a branch-free bulk phase (below the causal diagonal /
// inside the seq bound) and a masked diagonal+tail phase.
// ============================================================================

// one 32-key sub-tile (of the 64-row staged chunk) of the dQ loop.
// DROP: dS = P o (dP_d o M/(1-p) - D) — P stays undropped, the V^T dO
// term is masked+rescaled with the forward's published keep bits.
template <bool MASKED, bool DROP, int D>
DEVI void dq_tile(const short (&ldsK)[64][D + 8],
                  const short (&ldsVr)[64][D + 8],
                  int sub, int64_t kv0, int64_t seq, int64_t myq,
                  float scale, int causal, float mylse, float mydelta,
                  const bf16x8 (&qfrag)[D / 16],
                  const bf16x8 (&dofrag)[D / 16],
                  f32x16 (&dqt)[D / 32], int lq, int hi,
                  const unsigned int* maskrow, int64_t mask_w,
                  float inv_keep) {
  f32x16 st = {};
  f32x16 dpt = {};
#pragma unroll
  for (int c = 0; c < D / 16; ++c) {
    bf16x8 kf = *reinterpret_cast<const bf16x8*>(
        &ldsK[sub + lq][hi * 8 + 16 * c]);
    bf16x8 vf = *reinterpret_cast<const bf16x8*>(
        &ldsVr[sub + lq][hi * 8 + 16 * c]);
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
#pragma unroll
  for (int kc = 0; kc < 2; ++kc) {
    bf16x8 db = kc == 0 ? db0 : db1;
#pragma unroll
    for (int dj = 0; dj < D / 32; ++dj) {
      bf16x8 kt;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int kr = sub + kc * 16 + hi * 8 + j;
        kt[j] = ldsK[kr][dj * 32 + lq];
      }
      dqt[dj] =
          __builtin_amdgcn_mfma_f32_32x32x16_bf16(kt, db, dqt[dj], 0, 0, 0);
    }
  }
}

// new dQ tile body (see dv_tile_tr): K/V in the dual-use image, the
// K-transposed fragments by ds_read_b64_tr_b16, hardware bf16 convert.
// The row constants were lane-local already.
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
  bf16x8 db0 = assemble_pfrag<true>(&ds[0]);
  bf16x8 db1 = assemble_pfrag<true>(&ds[8]);
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

template <bool DROP, bool DBUF, int D, bool TR>
__global__ __launch_bounds__(256, D == 64 ? 3 : 2) void attn_bwd_dq_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, const short* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    short* __restrict__ dq, const short* __restrict__ out, int64_t seq,
    float scale, int causal, int64_t heads, int64_t in_sb, int64_t in_sh,
    int64_t in_ss, int64_t do_sb, int64_t do_sh, int64_t do_ss,
    int64_t g_sb, int64_t g_sh, int64_t g_ss, int64_t o_sb, int64_t o_sh,
    int64_t o_ss, const unsigned int* __restrict__ mask, int64_t mask_w,
    float inv_keep, const float* __restrict__ dlse,
    const int* __restrict__ seqlens) {
  constexpr int PITCH = TR ? img_pitch<D>() : D + 8;
  __shared__ __attribute__((aligned(16))) short
      ldsK[DBUF ? 2 : 1][64][PITCH];
  __shared__ __attribute__((aligned(16))) short
      ldsVr[DBUF ? 2 : 1][64][PITCH];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int hi = lane >> 5;
  const int lq = lane & 31;
  // causal: global longest-first packing; non-causal: XCD-local order
  // (see attn_fwd_kernel)
  const BlockPos pos = block_pos(causal, true);
  const int64_t bh = pos.bh;
  const int64_t q0_blk = pos.blk * 128;
  const int64_t q0 = q0_blk + wave * 32;
  const int64_t len = sample_len(seqlens, bh / heads, seq);
  const int64_t myq = q0 + lq;
  // padded query rows are zeroed ahead of the loop and a block wholly
  // inside the padding loads nothing (see attn_fwd_kernel); the delta of
  // padded rows stays unwritten — the dK kernel never reads it
  if (myq >= len && myq < seq)
    zero_row<D>(dq + (bh / heads) * g_sb + (bh % heads) * g_sh +
                    myq * g_ss, hi);
  if (q0_blk >= len) return;
  const bool active = q0 < len;
  const int64_t boff = (bh / heads) * in_sb + (bh % heads) * in_sh;
  const short* qp = q + boff;
  const short* kp = k + boff;
  const short* vp = v + boff;
  const short* dop = dout + (bh / heads) * do_sb + (bh % heads) * do_sh;

  const int64_t qrow = myq < len ? myq : len - 1;
  const float mylse = lse[bh * seq + qrow];

  const short* op_ = out + (bh / heads) * o_sb + (bh % heads) * o_sh;
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
  // D_i = rowsum(dO * O): this lane covers 32 of the 64 d-elements, the
  // partner lane (^32) the rest
  // dlse (ring-attention block merge): lse = logsumexp(S) has
  // dlse_i/dS_ij = P_ij, so an incoming lse gradient folds into the
  // per-row constant: dS = P o (dP - (D - dlse)).  The published delta
  // is pre-adjusted so the dK kernel needs no change.
  float mydelta = dsum + __shfl_xor(dsum, 32, 64);
  if (dlse != nullptr) mydelta -= dlse[bh * seq + qrow];
  // publish delta for the dK kernel that follows on the same stream
  if (myq < len && hi == 0)
    const_cast<float*>(delta)[bh * seq + myq] = mydelta;

  f32x16 dqt[D / 32] = {};

  const int stage_row = threadIdx.x >> 3;
  const int stage_seg = (threadIdx.x & 7) * 8;
  // bulk chunks (64 kv rows) are full for every lane; q0_blk is a
  // multiple of 128 so the causal bulk region is 64-aligned
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
            img_at<TR, D>(ldsK[0], stage_row + half * 32,
                          stage_seg + seg)) =
            *reinterpret_cast<const bf16x8*>(
                kp + kr * in_ss + stage_seg + seg);
        *reinterpret_cast<bf16x8*>(
            img_at<TR, D>(ldsVr[0], stage_row + half * 32,
                          stage_seg + seg)) =
            *reinterpret_cast<const bf16x8*>(
                vp + kr * in_ss + stage_seg + seg);
      }
    }
    __syncthreads();
  };

  // DBUF: same register-double-buffered single-barrier pipeline as the
  // dV/dK kernels (next kv chunk prefetched into VGPRs during this
  // chunk's MFMAs; see attn_bwd_dv_kernel).
  bf16x8 rk[2][D / 64], rv[2][D / 64];
  auto prefetch = [&](int64_t kv0) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      int64_t kr = kv0 + stage_row + half * 32;
      if (kr >= len) kr = len - 1;
#pragma unroll
      for (int s = 0; s < D / 64; ++s) {
        rk[half][s] = *reinterpret_cast<const bf16x8*>(
            kp + kr * in_ss + stage_seg + s * 64);
        rv[half][s] = *reinterpret_cast<const bf16x8*>(
            vp + kr * in_ss + stage_seg + s * 64);
      }
    }
  };
  auto commit = [&](int buf) {
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int s = 0; s < D / 64; ++s) {
        *reinterpret_cast<bf16x8*>(
            img_at<TR, D>(ldsK[buf], stage_row + half * 32,
                          stage_seg + s * 64)) =
            rk[half][s];
        *reinterpret_cast<bf16x8*>(
            img_at<TR, D>(ldsVr[buf], stage_row + half * 32,
                          stage_seg + s * 64)) =
            rv[half][s];
      }
  };

  const unsigned int* maskrow =
      DROP ? mask + bh * seq * mask_w : (const unsigned int*)nullptr;
  // one 32-key sub-tile from LDS buffer rb: new or legacy body
  auto tile = [&](auto masked, int rb, int sub, int64_t kvs) {
    constexpr bool M = decltype(masked)::value;
    if constexpr (TR)
      dq_tile_tr<M, DROP, D>(&ldsK[rb][0][0], &ldsVr[rb][0][0], sub, kvs,
                             len, myq, scale, causal, mylse, mydelta,
                             qfrag, dofrag, dqt, lq, hi, maskrow, mask_w,
                             inv_keep);
    else
      dq_tile<M, DROP, D>(ldsK[rb], ldsVr[rb], sub, kvs, len, myq, scale,
                          causal, mylse, mydelta, qfrag, dofrag, dqt, lq,
                          hi, maskrow, mask_w, inv_keep);
  };
  constexpr std::true_type MASKED_T{};
  constexpr std::false_type PLAIN_T{};
  if (!DBUF) {
    int64_t kv0 = 0;
    for (; kv0 < bulk_end; kv0 += 64) {
      stage_kv64(kv0);
#pragma unroll
      for (int sub = 0; sub < 64; sub += 32)
        tile(PLAIN_T, 0, sub, kv0 + sub);
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
        tile(MASKED_T, 0, sub, kvs);
      }
    }
  } else {
    int buf = 0;
    prefetch(0);
    for (int64_t kv0 = 0; kv0 < blk_kv_end; kv0 += 64) {
      commit(buf);
      __syncthreads();
      if (kv0 + 64 < blk_kv_end) prefetch(kv0 + 64);
      const int rb = buf;
      buf ^= 1;
      if (kv0 < bulk_end) {
#pragma unroll
        for (int sub = 0; sub < 64; sub += 32)
          tile(PLAIN_T, rb, sub, kv0 + sub);
      } else if (active) {
        const int64_t wave_kv_end = causal
            ? (q0 + 32 < len ? q0 + 32 : len) : len;
#pragma unroll
        for (int sub = 0; sub < 64; sub += 32) {
          const int64_t kvs = kv0 + sub;
          if (kvs >= wave_kv_end) break;
          tile(MASKED_T, rb, sub, kvs);
        }
      }
    }
  }

  if (!active || myq >= len) return;
  short* dqp = dq + (bh / heads) * g_sb + (bh % heads) * g_sh + myq * g_ss;
#pragma unroll
  for (int dj = 0; dj < D / 32; ++dj) {
    if constexpr (TR) {
      store_acc_bf16(dqp + dj * 32, dqt[dj], hi);
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        dqp[dj * 32 + crow(r, hi)] = (short)f2bf(dqt[dj][r]);
    }
  }
}

}  // namespace

extern "C" {

void epl_attn_fwd(const void* q, const void* k, const void* v, void* out,
                  float* lse, int64_t batch_heads, int64_t seq, float scale,
                  bool causal, int64_t heads, int64_t head_dim,
                  const int64_t* in_strides,
                  const int64_t* o_strides, unsigned int* drop_mask,
                  int64_t mask_w, unsigned long long seed, int drop_thresh,
                  float inv_keep, const int* seqlens, hipStream_t stream) {
  // causal: (x=bh, y=qblocks) — x-fastest dispatch launches every
  // batch-head of the longest q-block first (kernels read the mapping
  // from the causal flag)
  const unsigned nqb = (unsigned)((seq + 127) / 128);
  dim3 grid = causal ? dim3((unsigned)batch_heads, nqb)
                     : dim3(nqb, (unsigned)batch_heads);
#define FWD_ARGS                                                         \
  reinterpret_cast<const short*>(q), reinterpret_cast<const short*>(k),  \
      reinterpret_cast<const short*>(v), reinterpret_cast<short*>(out),  \
      lse, seq, scale, causal ? 1 : 0, heads, in_strides[0],             \
      in_strides[1], in_strides[2], o_strides[0], o_strides[1],          \
      o_strides[2], drop_mask, mask_w, seed, drop_thresh, inv_keep,      \
      seqlens
  if (head_dim == 128) {
    if (drop_mask != nullptr)
      hipLaunchKernelGGL(HIP_KERNEL_NAME(attn_fwd_kernel<true, 128>),
                         grid, dim3(256), 0, stream, FWD_ARGS);
    else
      hipLaunchKernelGGL(HIP_KERNEL_NAME(attn_fwd_kernel<false, 128>),
                         grid, dim3(256), 0, stream, FWD_ARGS);
  } else if (drop_mask != nullptr) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(attn_fwd_kernel<true, 64>), grid,
                       dim3(256), 0, stream, FWD_ARGS);
  } else {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(attn_fwd_kernel<false, 64>), grid,
                       dim3(256), 0, stream, FWD_ARGS);
  }
#undef FWD_ARGS
}

void epl_attn_bwd(const void* q, const void* k, const void* v,
                  const void* out, const void* dout, const float* lse,
                  float* delta_ws, void* dq, void* dk, void* dv,
                  int64_t batch_heads, int64_t seq, float scale,
                  bool causal, int64_t heads, const int64_t* in_strides,
                  const int64_t* o_strides, const int64_t* do_strides,
                  const int64_t* g_strides, int split_dkdv,
                  const unsigned int* drop_mask, int64_t mask_w,
                  float inv_keep, int64_t head_dim, const float* dlse,
                  const int* seqlens, hipStream_t stream) {
  const unsigned nqb = (unsigned)((seq + 127) / 128);
  dim3 grid = causal ? dim3((unsigned)batch_heads, nqb)
                     : dim3(nqb, (unsigned)batch_heads);
  // split_dkdv = 0 asks for the combined dK+dV kernel; it exists for d64,
  // non-causal, no dropout (with or without seqlens and dlse), and every
  // other call runs the split kernels whatever the flag says.
  const bool fused = !split_dkdv && drop_mask == nullptr &&
                     head_dim == 64 && !causal;
  {
    // split order: dV (needs no delta) -> dQ (computes + publishes delta
    // from the dO/O rows it already loads) -> dK (consumes delta).
    // Combined: dQ -> dK+dV.
#define DV_ARGS                                                         \
  reinterpret_cast<const short*>(q), reinterpret_cast<const short*>(k),  \
      reinterpret_cast<const short*>(dout), lse,                         \
      reinterpret_cast<short*>(dv), seq, scale, causal ? 1 : 0, heads,   \
      in_strides[0], in_strides[1], in_strides[2], do_strides[0],        \
      do_strides[1], do_strides[2], g_strides[0], g_strides[1],          \
      g_strides[2], drop_mask, mask_w, inv_keep, seqlens
#define DQ_ARGS                                                          \
  reinterpret_cast<const short*>(q), reinterpret_cast<const short*>(k),  \
      reinterpret_cast<const short*>(v),                                 \
      reinterpret_cast<const short*>(dout), lse, delta_ws,               \
      reinterpret_cast<short*>(dq), reinterpret_cast<const short*>(out), \
      seq, scale, causal ? 1 : 0, heads, in_strides[0], in_strides[1],   \
      in_strides[2], do_strides[0], do_strides[1], do_strides[2],        \
      g_strides[0], g_strides[1], g_strides[2], o_strides[0],            \
      o_strides[1], o_strides[2], drop_mask, mask_w, inv_keep, dlse,     \
      seqlens
#define DK_ARGS                                                          \
  reinterpret_cast<const short*>(q), reinterpret_cast<const short*>(k),  \
      reinterpret_cast<const short*>(v),                                 \
      reinterpret_cast<const short*>(dout), lse, delta_ws,               \
      reinterpret_cast<short*>(dk), seq, scale, causal ? 1 : 0, heads,   \
      in_strides[0], in_strides[1], in_strides[2], do_strides[0],        \
      do_strides[1], do_strides[2], g_strides[0], g_strides[1],          \
      g_strides[2], drop_mask, mask_w, inv_keep, seqlens
    // d64 staging mode (EPL_ATTN_BWD_DBUF): 0 = two-barrier direct
    // staging; 1 = dV double-buffered single-barrier pipeline
    // (spill-free); 2 = dK pipelined too (spills 12-40 VGPRs at 3
    // waves but still wins on long q loops); 3 = dQ pipelined too
    // (spills 68 B/lane at 3 waves).
    // Default -1 = auto: non-causal runs mode 2 (same-box A/B in
    // profiles/r02_dbuf_ab.txt: bert s512 -7.6%, s4096 -9.9%), causal
    // keeps direct staging (its per-block q loop is half as long and
    // mode 2 measured +2% there).  d128 keeps direct staging (doubled
    // LDS would cost its 2-waves occupancy).
    static const int dbuf_mode = [] {
      const char* e = getenv("EPL_ATTN_BWD_DBUF");
      return e == nullptr ? -1 : atoi(e);
    }();
    const int mode = dbuf_mode < 0 ? (causal ? 0 : 2) : dbuf_mode;
    const bool dbuf = mode >= 1;
    const bool dbuf_k = mode >= 2;
    const bool dbuf_q = mode >= 3;
    // tile bodies (EPL_ATTN_BWD_TILES): default = transposed-LDS-read
    // tiles; "legacy" = the previous bodies, kept for a same-process
    // A/B until a second independent run confirms the numbers
    static const bool legacy_tiles = [] {
      const char* e = getenv("EPL_ATTN_BWD_TILES");
      return e != nullptr && strcmp(e, "legacy") == 0;
    }();
    auto launch3 = [&](auto drop_c, auto d_c, auto tr_c) {
      constexpr bool DROP = decltype(drop_c)::value;
      constexpr int D = decltype(d_c)::value;
      constexpr bool TR = decltype(tr_c)::value;
      if (fused) {
        // nothing to launch ahead of dQ
      } else if (D == 64 && dbuf)
        hipLaunchKernelGGL(
            HIP_KERNEL_NAME(attn_bwd_dv_kernel<DROP, D == 64, D, TR>), grid,
            dim3(256), 0, stream, DV_ARGS);
      else
        hipLaunchKernelGGL(
            HIP_KERNEL_NAME(attn_bwd_dv_kernel<DROP, false, D, TR>), grid,
            dim3(256), 0, stream, DV_ARGS);
      if (D == 64 && dbuf_q)
        hipLaunchKernelGGL(
            HIP_KERNEL_NAME(attn_bwd_dq_kernel<DROP, D == 64, D, TR>), grid,
            dim3(256), 0, stream, DQ_ARGS);
      else
        hipLaunchKernelGGL(
            HIP_KERNEL_NAME(attn_bwd_dq_kernel<DROP, false, D, TR>), grid,
            dim3(256), 0, stream, DQ_ARGS);
      if (fused)
        hipLaunchKernelGGL(
            attn_bwd_dkdv_kernel, grid, dim3(256), 0, stream,
            reinterpret_cast<const short*>(q),
            reinterpret_cast<const short*>(k),
            reinterpret_cast<const short*>(v),
            reinterpret_cast<const short*>(dout), lse, delta_ws,
            reinterpret_cast<short*>(dk), reinterpret_cast<short*>(dv), seq,
            scale, heads, in_strides[0], in_strides[1], in_strides[2],
            do_strides[0], do_strides[1], do_strides[2], g_strides[0],
            g_strides[1], g_strides[2], seqlens);
      else if (D == 64 && dbuf_k)
        hipLaunchKernelGGL(
            HIP_KERNEL_NAME(attn_bwd_dk_kernel<DROP, D == 64, D, TR>), grid,
            dim3(256), 0, stream, DK_ARGS);
      else
        hipLaunchKernelGGL(
            HIP_KERNEL_NAME(attn_bwd_dk_kernel<DROP, false, D, TR>), grid,
            dim3(256), 0, stream, DK_ARGS);
    };
    auto launch2 = [&](auto drop_c, auto d_c) {
      if (legacy_tiles)
        launch3(drop_c, d_c, std::false_type{});
      else
        launch3(drop_c, d_c, std::true_type{});
    };
    using d64 = std::integral_constant<int, 64>;
    using d128 = std::integral_constant<int, 128>;
    if (head_dim == 128) {
      if (drop_mask != nullptr)
        launch2(std::true_type{}, d128{});
      else
        launch2(std::false_type{}, d128{});
    } else if (drop_mask != nullptr) {
      launch2(std::true_type{}, d64{});
    } else {
      launch2(std::false_type{}, d64{});
    }
#undef DV_ARGS
#undef DQ_ARGS
#undef DK_ARGS
  }
}

}  // extern "C"
