// Dual-use LDS image of a [64][D] bf16 tile for the attention kernels
// (the backward's new tile bodies; the forward's V tile, of which only
// the transposed read is used) and the tr_read_probe kernel that checks
// it.
//
// One copy of a Q / dO / K / V tile serves both kinds of MFMA operand read:
//  * row fragments, ds_read_b128 at [row][8*ch .. 8*ch+7];
//  * transposed fragments, two ds_read_b64_tr_b16 per bf16x8 operand.
// Every store and load goes through img_off, so the layout lives here
// only.
//
// Layout: plain rows padded to 72 (D=64) / 152 (D=128) shorts, so every
// address is one per-lane base plus an immediate.  By the 64-bank rule
// per lane group (table in docs/kernels.md) the ds_read_b128 row reads
// and the ds_write_b128 staging stores are conflict-free and the
// transposed read is 2-way (4 LDS cycles instead of 2).  An unpadded
// image with the chunk index XOR-ed by a row hash is conflict-free for
// all three; it measured the same kernel times and cost more address
// VGPRs in kernels that sit at their register limit (NOTES.md), so the
// padded rows stay.
#pragma once

#include <hip/hip_runtime.h>

namespace attn_img {

using s16x4 = __attribute__((ext_vector_type(4))) short;
using s16x8 = __attribute__((ext_vector_type(8))) short;

// row pitch in shorts
template <int D>
constexpr int img_pitch() { return D == 64 ? 72 : 152; }

// offset in shorts of 16-byte chunk ch (8 columns) of row `row`
template <int D>
__device__ __forceinline__ int img_off(int row, int ch) {
  return row * img_pitch<D>() + 8 * ch;
}

// A-operand fragment of the TRANSPOSED tile for v_mfma_f32_32x32x16_bf16:
// element j of lane l = img[r0 + 8*(l>>5) + j][32*dj + (l&31)].  Two
// ds_read_b64_tr_b16, four rows apart: in each 16-lane group, lane 4q+p
// supplies the address of row q, columns 4p..4p+3 of the group's 4x16
// block and lane i receives column i.  Needs EXEC all ones — call only
// from wave-uniform control flow, never under a per-lane test.
template <int D>
__device__ __forceinline__ s16x8 tr_frag(const short* img, int r0, int dj,
                                         int lane) {
  typedef s16x4 __attribute__((address_space(3))) lds_b64;
  const int row = r0 + 8 * (lane >> 5) + ((lane & 15) >> 2);
  const int ch = 4 * dj + 2 * ((lane >> 4) & 1) + ((lane & 3) >> 1);
  const int sub = 4 * (lane & 1);
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_b64*)(img + img_off<D>(row, ch) + sub));
  s16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_b64*)(img + img_off<D>(row + 4, ch) + sub));
  return __builtin_shufflevector(lo, hi4, 0, 1, 2, 3, 4, 5, 6, 7);
}

// the same fragment by eight 2-byte reads (the definition tr_frag must
// reproduce; what the legacy tile bodies do on their padded rows)
template <int D>
__device__ __forceinline__ s16x8 gather_frag(const short* img, int r0,
                                             int dj, int lane) {
  s16x8 out;
  const int col = 32 * dj + (lane & 31);
#pragma unroll
  for (int j = 0; j < 8; ++j)
    out[j] = img[img_off<D>(r0 + 8 * (lane >> 5) + j, col >> 3) + (col & 7)];
  return out;
}

}  // namespace attn_img
