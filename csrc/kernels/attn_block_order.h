// XCD-local block order of the non-causal attention grids.
//
// A non-causal launch is dim3(n, BH): n 128-row blocks per batch-head on
// x, the batch-heads on y.  The n blocks of one batch-head read the same
// operands (the forward and dQ blocks the head's K and V, the dV/dK
// blocks its Q and dO).  Blocks are handed out x-fastest and round-robin
// over the 8 XCDs, so with (bh, blk) = (blockIdx.y, blockIdx.x) the
// blocks of a head sit on different XCDs and every private L2 fetches the
// head's operands for itself.  block_of() deals the work differently:
// from the linear id L = blockIdx.x + n * blockIdx.y, the blocks with the
// same L % 8 (which share an XCD) take, in the order of L / 8, all the
// blocks of one head and then those of the next.
//
//   BH8 = BH & ~7
//   L <  n * BH8:  g = L % 8, i = L / 8:  blk = i % n, bh = (i / n) * 8 + g
//   L >= n * BH8:  bh = L / n, blk = L % n                    (identity)
//
// Bijection onto [0, BH) x [0, n), for every n >= 1 and BH >= 1:
//  * n * BH8 is a multiple of 8, so the ids below it are exactly the
//    pairs (g, i) with 0 <= g < 8 and 0 <= i < n * BH8 / 8, one id each
//    (L = 8 i + g).  Write i = n t + blk with 0 <= blk < n; then
//    0 <= t < BH8 / 8 and bh = 8 t + g runs over [0, BH8).  The map
//    (g, t, blk) -> (bh, blk) has the inverse g = bh % 8, t = bh / 8, so
//    the ids below n * BH8 cover [0, BH8) x [0, n) once each.
//  * the ids from n * BH8 to n * BH - 1 keep (L / n, L % n), which covers
//    [BH8, BH) x [0, n) once each.
// It is an index permutation only: which block computes which tile
// changes, no arithmetic does, and nothing depends on where a block
// really runs — a different placement costs speed, never a result.
//
// The ids fit 32 bits: n and BH are grid dimensions (x holds n, at most
// 65535 by the binding's check; y at most 65535), and 65535 * 65535 <
// 2^32.  All inputs are block-uniform, so bh and blk stay in SGPRs.
// The causal grids keep their own axis order (longest-first packing).
#pragma once

#include <hip/hip_runtime.h>

namespace attn_order {

struct Block {
  unsigned int bh, blk;
};

__host__ __device__ inline Block block_of(unsigned int x, unsigned int y,
                                          unsigned int n, unsigned int BH) {
  const unsigned int L = x + n * y;
  const unsigned int BH8 = BH & ~7u;
  Block b;
  if (L < n * BH8) {
    const unsigned int g = L & 7u, i = L >> 3;
    b.blk = i % n;
    b.bh = (i / n) * 8u + g;
  } else {
    b.bh = L / n;
    b.blk = L % n;
  }
  return b;
}

}  // namespace attn_order
