// LDS images of the grouped expert GEMM (moe_gemm.hip): one 128 x 64 bf16
// operand tile per image, 16 KiB, unpadded, the 16-byte chunk index XOR-ed
// with a row hash.  Every store and load goes through row_off / tr_off,
// so the layouts live here only.
//
// An MFMA operand fragment of v_mfma_f32_32x32x16_bf16 is, for both
// operands, "lane l holds index i = l % 32 and the 8 contraction elements
// 8 * (l / 32) .. + 7".  Which LDS read forms it depends on which index is
// contiguous in memory, and the tile is staged as it lies in memory:
//
//  * ROW image [128 idx][64 r] (r contiguous: A of nn, both operands of
//    nt).  off = idx * 64 + 8 * (ch ^ ((idx >> 1) & 7)).  A fragment is one
//    ds_read_b128 at chunk 2 c + hi of row idx.  Rows are 128 B apart, so
//    rows 2 j and 2 j + 1 cover the two halves of the 64 banks and the
//    hash (idx >> 1) & 7 spreads 8 row pairs over the 8 chunks: 16
//    consecutive rows reading the same logical chunk touch 16 different
//    16-byte bank groups, as do the staging stores (8 lanes per row, 8
//    different chunks).
//
//  * TR image [64 r][128 idx] (idx contiguous: B of nn, both operands of
//    tn).  off = r * 128 + 8 * (ch ^ (4 * (r & 3))).  A fragment is two
//    ds_read_b64_tr_b16 four rows apart, with the lane map of
//    attn_img::tr_frag (attn_lds_image.h), restated here for a [64][128]
//    tile: in each 16-lane group lane 4 q + p supplies the address of row
//    q, columns 4 p .. 4 p + 3 of the group's 4 x 16 block, and lane i
//    receives column i.  A row is 256 B, all 64 banks, so without the hash
//    the 8 rows of one read (q = 0..3, two halves) collide 8-way; the hash
//    moves row q by q * 64 B, which leaves the two halves on the same
//    banks: 2-way, what the padded attention image has.  r & 3 is the same
//    for rows r and r + 4, so the second read is the first plus an
//    immediate.  Needs EXEC all ones: wave-uniform control flow only.
#pragma once

#include <hip/hip_runtime.h>

namespace moe_img {

using s16x4 = __attribute__((ext_vector_type(4))) short;
using s16x8 = __attribute__((ext_vector_type(8))) short;

constexpr int kTileShorts = 128 * 64;   // one operand image

// offset in shorts of 16-byte chunk ch (0..7) of row idx (0..127)
__device__ __forceinline__ int row_off(int idx, int ch) {
  return idx * 64 + 8 * (ch ^ ((idx >> 1) & 7));
}

// offset in shorts of 16-byte chunk ch (0..15) of contraction row r (0..63)
__device__ __forceinline__ int tr_off(int r, int ch) {
  return r * 128 + 8 * (ch ^ (4 * (r & 3)));
}

// element j of lane l = tile[idx = i0 + l % 32][r = 16 c + 8 (l / 32) + j]
__device__ __forceinline__ s16x8 row_frag(const short* img, int i0, int c,
                                          int lane) {
  return *reinterpret_cast<const s16x8*>(
      img + row_off(i0 + (lane & 31), 2 * c + (lane >> 5)));
}

// the same element from a TR image, tile[r][idx]; i0 a multiple of 32
__device__ __forceinline__ s16x8 tr_frag(const short* img, int i0, int c,
                                         int lane) {
  typedef s16x4 __attribute__((address_space(3))) lds_b64;
  const int r = 16 * c + 8 * (lane >> 5) + ((lane & 15) >> 2);
  const int col = i0 + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
  const short* p = img + tr_off(r, col >> 3) + (col & 7);
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_b64*)p);
  s16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_b64*)(p + 4 * 128));
  return __builtin_shufflevector(lo, hi4, 0, 1, 2, 3, 4, 5, 6, 7);
}

}  // namespace moe_img
