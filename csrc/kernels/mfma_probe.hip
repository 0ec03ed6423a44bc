// MFMA fragment-layout probe for v_mfma_f32_32x32x16_bf16 on gfx950.
// Computes D = A(32x16) x B(16x32) with the hypothesized lane->element
// maps and writes D to global memory; the host compares against a CPU
// reference (asymmetric A and B so transposes are caught).
//
// Hypothesized layouts (CDNA3 32x32x8 pattern with K doubled):
//   A[m][k]: lane l holds m = l%32, k = (l/32)*8 + j   (j = 0..7)
//   B[k][n]: lane l holds n = l%32, k = (l/32)*8 + j
//   C/D    : col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
//            (authoritative, cdna_hip_programming.md section 3)

#include <hip/hip_runtime.h>

#include "attn_block_order.h"
#include "attn_lds_image.h"

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x16 = __attribute__((ext_vector_type(16))) float;

__global__ void mfma_probe_kernel(const unsigned short* __restrict__ A,
                                  const unsigned short* __restrict__ B,
                                  float* __restrict__ D) {
  const int lane = threadIdx.x & 63;
  const int half = lane >> 5;     // 0 or 1
  const int lm = lane & 31;
  bf16x8 a, b;
  for (int j = 0; j < 8; ++j) {
    // A is 32x16 row-major; B is 16x32 row-major
    a[j] = (short)A[lm * 16 + (half * 8 + j)];
    b[j] = (short)B[(half * 8 + j) * 32 + lm];
  }
  f32x16 c = {};
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  for (int reg = 0; reg < 16; ++reg) {
    const int row = (reg & 3) + 8 * (reg >> 2) + 4 * half;
    const int col = lm;
    D[row * 32 + col] = c[reg];
  }
}

extern "C" void run_mfma_probe(const unsigned short* A,
                               const unsigned short* B, float* D,
                               hipStream_t stream) {
  hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0, stream, A, B,
                     D);
}

// Transposed-LDS-read probe: one wave fills the attention backward's
// dual-use [64][D] image with index-coded values row*256+col, then forms
// every transposed A-operand fragment the tiles use — (sub, qc, dj) —
// both ways: by eight 2-byte reads (the definition) and by two
// ds_read_b64_tr_b16.  out_*[frag][lane][j], frag = (sub/32*2+qc)*(D/32)+dj.
template <int D>
__global__ void tr_read_probe_kernel(short* __restrict__ out_gather,
                                     short* __restrict__ out_tr) {
  __shared__ __attribute__((aligned(16))) short
      img[64 * attn_img::img_pitch<D>()];
  const int lane = threadIdx.x & 63;
  for (int i = lane; i < 64 * D; i += 64) {
    const int row = i / D, col = i % D;
    img[attn_img::img_off<D>(row, col >> 3) + (col & 7)] =
        (short)(row * 256 + col);
  }
  __syncthreads();
  for (int sub = 0; sub < 64; sub += 32)
    for (int qc = 0; qc < 2; ++qc)
      for (int dj = 0; dj < D / 32; ++dj) {
        const int frag = ((sub >> 5) * 2 + qc) * (D / 32) + dj;
        const bf16x8 g =
            attn_img::gather_frag<D>(img, sub + qc * 16, dj, lane);
        const bf16x8 t = attn_img::tr_frag<D>(img, sub + qc * 16, dj, lane);
        *reinterpret_cast<bf16x8*>(out_gather + (frag * 64 + lane) * 8) = g;
        *reinterpret_cast<bf16x8*>(out_tr + (frag * 64 + lane) * 8) = t;
      }
}

extern "C" void run_tr_read_probe(short* out_gather, short* out_tr,
                                  int head_dim, hipStream_t stream) {
  if (head_dim == 128)
    hipLaunchKernelGGL(tr_read_probe_kernel<128>, dim3(1), dim3(64), 0,
                       stream, out_gather, out_tr);
  else
    hipLaunchKernelGGL(tr_read_probe_kernel<64>, dim3(1), dim3(64), 0,
                       stream, out_gather, out_tr);
}

// Block-order probe: launched on a non-causal attention grid dim3(n, BH),
// every block writes the (bh, blk) that attn_order::block_of gives it at
// its linear id L = blockIdx.x + n * blockIdx.y.  out: int32 [n * BH][2].
__global__ void block_order_probe_kernel(int* __restrict__ out) {
  if (threadIdx.x != 0) return;
  const attn_order::Block b =
      attn_order::block_of(blockIdx.x, blockIdx.y, gridDim.x, gridDim.y);
  const unsigned int L = blockIdx.x + gridDim.x * blockIdx.y;
  out[2 * (size_t)L] = (int)b.bh;
  out[2 * (size_t)L + 1] = (int)b.blk;
}

extern "C" void run_block_order_probe(int* out, int n, int bh,
                                      hipStream_t stream) {
  hipLaunchKernelGGL(block_order_probe_kernel, dim3(n, bh), dim3(64), 0,
                     stream, out);
}
