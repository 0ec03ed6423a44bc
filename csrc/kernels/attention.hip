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
// All kernels take (batch, head, seq) strides so the qkv-unbind views are
// consumed without copies.
//
// Non-causal grids run in the XCD-local block order of
// attn_block_order.h: the 128-row blocks of a batch-head, which read the
// same operands, share one L2 instead of fetching them once per XCD.

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>
#include <type_traits>

#include "attn_block_order.h"
#include "attn_lds_image.h"

#include "attn_tiles.h"

namespace {

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

// attention_gqa.hip holds this kernel's grouped-query twin
// (attn_fwd_gqa_kernel): a fix to one belongs in the other
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

template <bool DROP, bool DBUF, int D>
__global__ __launch_bounds__(256, D == 64 ? (DBUF ? 3 : 4)
                                          : (!DROP ? 3 : 2))
void attn_bwd_dv_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ dout, const float* __restrict__ lse,
    short* __restrict__ dv, int64_t seq, float scale, int causal,
    int64_t heads, int64_t in_sb, int64_t in_sh, int64_t in_ss,
    int64_t do_sb, int64_t do_sh, int64_t do_ss, int64_t g_sb,
    int64_t g_sh, int64_t g_ss,
    const unsigned int* __restrict__ mask, int64_t mask_w,
    float inv_keep, const int* __restrict__ seqlens) {
  // dual-use image + the chunk's 64 -lse/scale values
  constexpr int PITCH = img_pitch<D>();
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
  float rl = 0.f;   // wave 0 carries the chunk's -lse/scale values
  const float neg_inv_scale = -1.f / scale;
  auto prefetch = [&](int64_t q0) {
    if (wave == 0) {
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
    if (wave == 0) ldsL[buf][lane] = rl;
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int s = 0; s < D / 64; ++s) {
        *reinterpret_cast<bf16x8*>(
            img_at<D>(ldsQ[buf], stage_row + half * 32,
                      stage_seg + s * 64)) =
            rq[half][s];
        *reinterpret_cast<bf16x8*>(
            img_at<D>(ldsDO[buf], stage_row + half * 32,
                      stage_seg + s * 64)) =
            rdo[half][s];
      }
  };
  auto stage_q64 = [&](int64_t q0) {
    __syncthreads();
    if (wave == 0) {
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
            img_at<D>(ldsQ[0], stage_row + half * 32,
                      stage_seg + seg)) =
            *reinterpret_cast<const bf16x8*>(
                qp + qr * in_ss + stage_seg + seg);
        *reinterpret_cast<bf16x8*>(
            img_at<D>(ldsDO[0], stage_row + half * 32,
                      stage_seg + seg)) =
            *reinterpret_cast<const bf16x8*>(
                dop + qr * do_ss + stage_seg + seg);
      }
    }
    __syncthreads();
  };

  const unsigned int* maskrow =
      DROP ? mask + bh * seq * mask_w : (const unsigned int*)nullptr;
  // one 32-row sub-tile from LDS buffer rb
  auto tile = [&](auto masked, int rb, int sub, int64_t q0s) {
    constexpr bool M = decltype(masked)::value;
    dv_tile_tr<M, DROP, D>(&ldsQ[rb][0][0], &ldsDO[rb][0][0],
                           &ldsL[rb][sub], sub, q0s, len, mykv, scale,
                           causal, kfrag, dvt, lkv, hi, maskrow, mask_w,
                           inv_keep);
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
  for (int dj = 0; dj < D / 32; ++dj)
    store_acc_bf16(dvp + dj * 32, dvt[dj], hi);
}

template <bool DROP, bool DBUF, int D>
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
  constexpr int PITCH = img_pitch<D>();
  __shared__ __attribute__((aligned(16))) short
      ldsQ[DBUF ? 2 : 1][64][PITCH];
  __shared__ __attribute__((aligned(16))) short
      ldsDO[DBUF ? 2 : 1][64][PITCH];
  // [0] = -lse/scale, [1] = -delta of the chunk's 64 rows
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
  float rl = 0.f;   // wave 0 carries -lse/scale, wave 1 -delta
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
    if (wave < 2) ldsL[buf][wave][lane] = rl;
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int s = 0; s < D / 64; ++s) {
        *reinterpret_cast<bf16x8*>(
            img_at<D>(ldsQ[buf], stage_row + half * 32,
                      stage_seg + s * 64)) =
            rq[half][s];
        *reinterpret_cast<bf16x8*>(
            img_at<D>(ldsDO[buf], stage_row + half * 32,
                      stage_seg + s * 64)) =
            rdo[half][s];
      }
  };
  auto stage_q64 = [&](int64_t q0) {
    __syncthreads();
    if (wave < 2) {
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
            img_at<D>(ldsQ[0], stage_row + half * 32,
                      stage_seg + seg)) =
            *reinterpret_cast<const bf16x8*>(
                qp + qr * in_ss + stage_seg + seg);
        *reinterpret_cast<bf16x8*>(
            img_at<D>(ldsDO[0], stage_row + half * 32,
                      stage_seg + seg)) =
            *reinterpret_cast<const bf16x8*>(
                dop + qr * do_ss + stage_seg + seg);
      }
    }
    __syncthreads();
  };

  const unsigned int* maskrow =
      DROP ? mask + bh * seq * mask_w : (const unsigned int*)nullptr;
  // one 32-row sub-tile from LDS buffer rb
  auto tile = [&](auto masked, int rb, int sub, int64_t q0s) {
    constexpr bool M = decltype(masked)::value;
    dk_tile_tr<M, DROP, D>(&ldsQ[rb][0][0], &ldsDO[rb][0][0],
                           &ldsL[rb][0][sub], &ldsL[rb][1][sub], sub,
                           q0s, len, mykv, scale, causal, kfrag, vfrag,
                           dkt, lkv, hi, maskrow, mask_w, inv_keep);
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
  for (int dj = 0; dj < D / 32; ++dj)
    store_acc_bf16(dkp + dj * 32, dkt[dj], hi);
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
  bf16x8 pb0 = assemble_pfrag(&p[0]);
  bf16x8 pb1 = assemble_pfrag(&p[8]);
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
  bf16x8 db0 = assemble_pfrag(&ds[0]);
  bf16x8 db1 = assemble_pfrag(&ds[8]);
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
// backward kernel B (q-parallel): dQ.  K and V tiles staged in LDS in
// the dual-use image per block; row fragments via ds_read_b128,
// K-transposed fragments via ds_read_b64_tr_b16.  Like the forward, the
// kv loop is split into a branch-free bulk phase (below the causal
// diagonal / inside the seq bound) and a masked diagonal+tail phase.
// ============================================================================

// attention_gqa.hip holds this kernel's grouped-query twin
// (attn_bwd_dq_gqa_kernel): a fix to one belongs in the other
template <bool DROP, int D>
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
  __shared__ __attribute__((aligned(16))) short ldsK[64][img_pitch<D>()];
  __shared__ __attribute__((aligned(16))) short ldsVr[64][img_pitch<D>()];
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
            img_at<D>(ldsK, stage_row + half * 32, stage_seg + seg)) =
            *reinterpret_cast<const bf16x8*>(
                kp + kr * in_ss + stage_seg + seg);
        *reinterpret_cast<bf16x8*>(
            img_at<D>(ldsVr, stage_row + half * 32, stage_seg + seg)) =
            *reinterpret_cast<const bf16x8*>(
                vp + kr * in_ss + stage_seg + seg);
      }
    }
    __syncthreads();
  };

  const unsigned int* maskrow =
      DROP ? mask + bh * seq * mask_w : (const unsigned int*)nullptr;
  // one 32-key sub-tile of the staged chunk
  auto tile = [&](auto masked, int sub, int64_t kvs) {
    constexpr bool M = decltype(masked)::value;
    dq_tile_tr<M, DROP, D>(&ldsK[0][0], &ldsVr[0][0], sub, kvs, len, myq,
                           scale, causal, mylse, mydelta, qfrag, dofrag,
                           dqt, lq, hi, maskrow, mask_w, inv_keep);
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
  short* dqp = dq + (bh / heads) * g_sb + (bh % heads) * g_sh + myq * g_ss;
#pragma unroll
  for (int dj = 0; dj < D / 32; ++dj)
    store_acc_bf16(dqp + dj * 32, dqt[dj], hi);
}

}  // namespace

extern "C" {

// attention_gqa.hip
void epl_attn_fwd_gqa(const void*, const void*, const void*, void*, float*,
                      int64_t, int64_t, float, bool, int64_t, int64_t,
                      int64_t, const int64_t*, const int64_t*,
                      const int64_t*, const int*, hipStream_t);
void epl_attn_bwd_gqa(const void*, const void*, const void*, const void*,
                      const void*, const float*, float*, void*, void*, void*,
                      int64_t, int64_t, float, bool, int64_t, int64_t,
                      int64_t, const int64_t*, const int64_t*,
                      const int64_t*, const int64_t*, const int64_t*,
                      const int64_t*, const int*, hipStream_t);

void epl_attn_fwd(const void* q, const void* k, const void* v, void* out,
                  float* lse, int64_t batch_heads, int64_t seq, float scale,
                  bool causal, int64_t heads, int64_t head_dim,
                  const int64_t* in_strides,
                  const int64_t* o_strides, unsigned int* drop_mask,
                  int64_t mask_w, unsigned long long seed, int drop_thresh,
                  float inv_keep, const int* seqlens, int64_t kv_heads,
                  const int64_t* kv_strides, hipStream_t stream) {
  if (kv_heads != heads) {
    // grouped-query call (attention_gqa.hip); the binding refuses dropout
    epl_attn_fwd_gqa(q, k, v, out, lse, batch_heads, seq, scale, causal,
                     heads, kv_heads, head_dim, in_strides, kv_strides,
                     o_strides, seqlens, stream);
    return;
  }
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
                  const int* seqlens, int64_t kv_heads,
                  const int64_t* kv_strides, const int64_t* gkv_strides,
                  hipStream_t stream) {
  if (kv_heads != heads) {
    // grouped-query call (attention_gqa.hip): always the split kernels;
    // the binding refuses dropout and dlse
    epl_attn_bwd_gqa(q, k, v, out, dout, lse, delta_ws, dq, dk, dv,
                     batch_heads, seq, scale, causal, heads, kv_heads,
                     head_dim, in_strides, kv_strides, o_strides, do_strides,
                     g_strides, gkv_strides, seqlens, stream);
    return;
  }
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
    // (spill-free); 2 (or more) = dK pipelined too (spills 12-40 VGPRs
    // at 3 waves but still wins on long q loops).  dQ always stages
    // directly: its pipelined form lost both A/Bs
    // (profiles/r02_dbuf_ab.txt).
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
    auto launch = [&](auto drop_c, auto d_c) {
      constexpr bool DROP = decltype(drop_c)::value;
      constexpr int D = decltype(d_c)::value;
      if (fused) {
        // nothing to launch ahead of dQ
      } else if (D == 64 && dbuf)
        hipLaunchKernelGGL(
            HIP_KERNEL_NAME(attn_bwd_dv_kernel<DROP, D == 64, D>), grid,
            dim3(256), 0, stream, DV_ARGS);
      else
        hipLaunchKernelGGL(
            HIP_KERNEL_NAME(attn_bwd_dv_kernel<DROP, false, D>), grid,
            dim3(256), 0, stream, DV_ARGS);
      hipLaunchKernelGGL(HIP_KERNEL_NAME(attn_bwd_dq_kernel<DROP, D>), grid,
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
            HIP_KERNEL_NAME(attn_bwd_dk_kernel<DROP, D == 64, D>), grid,
            dim3(256), 0, stream, DK_ARGS);
      else
        hipLaunchKernelGGL(
            HIP_KERNEL_NAME(attn_bwd_dk_kernel<DROP, false, D>), grid,
            dim3(256), 0, stream, DK_ARGS);
    };
    using d64 = std::integral_constant<int, 64>;
    using d128 = std::integral_constant<int, 128>;
    if (head_dim == 128) {
      if (drop_mask != nullptr)
        launch(std::true_type{}, d128{});
      else
        launch(std::false_type{}, d128{});
    } else if (drop_mask != nullptr) {
      launch(std::true_type{}, d64{});
    } else {
      launch(std::false_type{}, d64{});
    }
#undef DV_ARGS
#undef DQ_ARGS
#undef DK_ARGS
  }
}

}  // extern "C"
