// Hidden-stream dropout inside the LayerNorm kernels (gfx950):
//
//   forward   s = D(x) (+ res),  y = LN(s) * gamma + beta
//   backward  g = LN-backward of dy (+ dy2) at the saved s (+ dadd)
//             d_res = g,  d_x = keep ? g * inv_keep : 0,  colsum over d_x
//   D(x)[r, c] = keep(r, c) ? x[r, c] * inv_keep : 0
//
// and the stand-alone pair out = D(x) (+ res) / dx = D(g) for the sites with
// no LayerNorm behind them.
//
// No mask tensor exists: keep(r, c) is a pure function of (seed, row,
// column) that every kernel here evaluates for itself.  One philox4x32-10
// call with counter (row lo, row hi, c >> 4, 0) and key (seed lo, seed hi)
// yields 16 bytes, numbered in word order, low byte first; element (r, c)
// is kept iff byte c & 15 is >= thresh.  Nothing in the keying knows the
// block size, CHUNKS, the presence of a residual or the kernel, so the
// block-per-row forward, the wave-per-row backward and the flat
// dropout_add kernels agree on every element.
//
// A lane owns 8 consecutive columns (one 16-byte access of bf16), i.e. half
// a philox call.  It makes ONE CALL PER 8 COLUMNS AND USES HALF of it: the
// pair of words (c >> 3) & 1 picks.  Sharing a call between the two lanes
// of a 16-column group would halve the calls only if the partner lane did
// other work meanwhile, which in a SIMD it cannot; pairing chunks would tie
// the mask to CHUNKS.  Cost: a call is 10 rounds of 2 v_mul_hi_u32 +
// 2 v_mul_lo_u32 + 2 v_xor3 (the key schedule is uniform and runs on the
// SALU), 60 VALU instructions, and the 8 byte tests add about 24; per row
// that is cols / 512 wave-level calls (2 at cols = 1024) next to the
// row's 8 * cols bytes of traffic.  The pivot's column-0 draw has uniform
// operands and is computed on the scalar unit.
//
// The forward applies the drop in one fma, s32 = fma(x, inv_keep, res):
// one fp32 rounding of the exact D(x) + res, as the plain kernel's
// s32 = x + res.

#include <hip/hip_runtime.h>
#include <cstdint>

#include "attn_tiles.h"   // philox4x32, cvt_pk_bf16 (read-only)

namespace {

using T = unsigned short;

struct float8 {
  float v[8];
};

DEVI float bfu2f(T u) { return __uint_as_float((unsigned int)u << 16); }

DEVI float8 load_bf16x8(const T* p) {
  const uint4 raw = *reinterpret_cast<const uint4*>(p);
  const unsigned int w[4] = {raw.x, raw.y, raw.z, raw.w};
  float8 f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f.v[2 * i] = __uint_as_float(w[i] << 16);
    f.v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
  return f;
}

DEVI void store_bf16x8(T* p, const float8& f) {
  *reinterpret_cast<uint4*>(p) =
      make_uint4(cvt_pk_bf16(f.v[0], f.v[1]), cvt_pk_bf16(f.v[2], f.v[3]),
                 cvt_pk_bf16(f.v[4], f.v[5]), cvt_pk_bf16(f.v[6], f.v[7]));
}

DEVI float8 load_f32x8(const float* p) {
  float8 f;
  const float4 a = *reinterpret_cast<const float4*>(p);
  const float4 b = *reinterpret_cast<const float4*>(p + 4);
  f.v[0] = a.x; f.v[1] = a.y; f.v[2] = a.z; f.v[3] = a.w;
  f.v[4] = b.x; f.v[5] = b.y; f.v[6] = b.z; f.v[7] = b.w;
  return f;
}

DEVI void store_f32x8(float* p, const float8& f) {
  *reinterpret_cast<float4*>(p) = make_float4(f.v[0], f.v[1], f.v[2], f.v[3]);
  *reinterpret_cast<float4*>(p + 4) =
      make_float4(f.v[4], f.v[5], f.v[6], f.v[7]);
}

// what every kernel needs to evaluate keep(r, c)
struct Drop {
  unsigned int k0, k1;   // seed lo, hi
  int thresh;            // a philox byte >= thresh keeps
  float inv_keep;
};

// the 8 philox bytes of columns c .. c+7 (c % 8 == 0) of a row
struct KeepBytes {
  unsigned int w[2];
  DEVI bool keep(int j, int thresh) const {
    return (int)((w[j >> 2] >> ((j & 3) * 8)) & 0xffu) >= thresh;
  }
  // the 8 decisions as one word, bit j = keep(j)
  DEVI unsigned int mask(int thresh) const {
    unsigned int m = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) m |= (unsigned int)keep(j, thresh) << j;
    return m;
  }
};

DEVI KeepBytes keep_bytes(int64_t row, int64_t c, const Drop& d) {
  unsigned int o[4];
  philox4x32((unsigned int)row, (unsigned int)((uint64_t)row >> 32),
             (unsigned int)(c >> 4), 0u, d.k0, d.k1, o);
  const bool hi = (c >> 3) & 1;
  return {{hi ? o[2] : o[0], hi ? o[3] : o[1]}};
}

// ---- block-wide sum (<= 256 threads), as the plain LN forward's -----------
DEVI float block_reduce_sum(float val, float* lds /* >= 4 floats */) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) val += __shfl_down(val, off, 64);
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int nwaves = blockDim.x >> 6;
  if (lane == 0) lds[wave] = val;
  __syncthreads();
  if (wave == 0) {
    val = lane < nwaves ? lds[lane] : 0.f;
#pragma unroll
    for (int off = 2; off > 0; off >>= 1) val += __shfl_down(val, off, 64);
    if (lane == 0) lds[0] = val;
  }
  __syncthreads();
  return lds[0];
}

// ============================================================================
// Forward: the register-cached one-pass LN forward (one block per row, pivot
// mean, variance out of the cached row, CHUNKS 1 / 2) with the drop applied
// to x in registers before the residual add.  s is ALWAYS written: the
// backward normalizes against it (without a residual s = D(x)).
// ============================================================================
template <bool HAS_RES, int CHUNKS>
__global__ void layer_norm_dropout_fwd_kernel(
    T* __restrict__ out, const T* __restrict__ x, const T* __restrict__ res,
    T* __restrict__ sum_out, const T* __restrict__ gamma,
    const T* __restrict__ beta, float* __restrict__ mean_out,
    float* __restrict__ rstd_out, int64_t rows, int64_t cols, float eps,
    Drop dp) {
  __shared__ float lds[8];
  float8 cache[CHUNKS];
  float8 gw[CHUNKS], bw[CHUNKS];
#pragma unroll
  for (int k = 0; k < CHUNKS; ++k) {
    const int64_t c = ((int64_t)threadIdx.x + k * blockDim.x) * 8;
    if (c < cols) {
      gw[k] = load_bf16x8(gamma + c);
      bw[k] = load_bf16x8(beta + c);
    }
  }
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int64_t base = row * cols;
    // pivot = s32 of column 0, formed by every thread from uniform
    // operands (one broadcast load each, the draw on the scalar unit)
    const bool keep0 = keep_bytes(row, 0, dp).keep(0, dp.thresh);
    const float r0 = HAS_RES ? bfu2f(res[base]) : 0.f;
    const float piv =
        keep0 ? __builtin_fmaf(bfu2f(x[base]), dp.inv_keep, r0) : r0;
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < CHUNKS; ++k) {
      const int64_t c = ((int64_t)threadIdx.x + k * blockDim.x) * 8;
      if (c >= cols) continue;
      float8 f = load_bf16x8(x + base + c);
      float8 r;
      if (HAS_RES) r = load_bf16x8(res + base + c);
      const KeepBytes kb = keep_bytes(row, c, dp);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float rv = HAS_RES ? r.v[j] : 0.f;
        f.v[j] = kb.keep(j, dp.thresh)
                     ? __builtin_fmaf(f.v[j], dp.inv_keep, rv)
                     : rv;
      }
      store_bf16x8(sum_out + base + c, f);
      cache[k] = f;
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += f.v[j] - piv;
    }
    sum = block_reduce_sum(sum, lds);
    const float mean = piv + sum / cols;
    float ssq = 0.f;
#pragma unroll
    for (int k = 0; k < CHUNKS; ++k) {
      const int64_t c = ((int64_t)threadIdx.x + k * blockDim.x) * 8;
      if (c >= cols) continue;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = cache[k].v[j] - mean;
        ssq += d * d;
      }
    }
    __syncthreads();
    ssq = block_reduce_sum(ssq, lds);
    const float rstd = rsqrtf(ssq / cols + eps);
    if (threadIdx.x == 0) {
      mean_out[row] = mean;
      rstd_out[row] = rstd;
    }
#pragma unroll
    for (int k = 0; k < CHUNKS; ++k) {
      const int64_t c = ((int64_t)threadIdx.x + k * blockDim.x) * 8;
      if (c >= cols) continue;
      float8 y;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        y.v[j] = (cache[k].v[j] - mean) * rstd * gw[k].v[j] + bw[k].v[j];
      store_bf16x8(out + base + c, y);
    }
    __syncthreads();
  }
}

// ============================================================================
// Backward: the one-row-per-wave fast backward (no barrier in the row loop,
// dgamma / dbeta / colsum accumulated in registers across the wave's rows,
// one partial row per block and plane, fixed-order reduce below) writing
// TWO tensors: d_res = g and d_x = keep ? g * inv_keep : 0, each rounded
// once from fp32.  The colsum plane sums the fp32 d_x.  DADD / COLSUM / DY2
// and the gamma placements (fp32 registers, packed bf16 registers at
// CHUNKS = 1, LDS at CHUNKS = 4) are the plain kernel's, and so are the
// waves-per-SIMD bounds; the draw happens in the second pass, right before
// the stores, so its temporaries do not live across the row reduction.
// ============================================================================
template <int CHUNKS, bool CACHE, bool DADD, bool COLSUM, bool DY2>
__global__ __launch_bounds__(256, CHUNKS == 1 ? 5 : 3) void
layer_norm_dropout_bwd_kernel(
    T* __restrict__ d_x, T* __restrict__ d_res, float* __restrict__ dg_part,
    float* __restrict__ db_part, float* __restrict__ cs_part,
    const T* __restrict__ dy, const T* __restrict__ dy2,
    const T* __restrict__ s, const T* __restrict__ gamma,
    const T* __restrict__ dadd, const float* __restrict__ mean_in,
    const float* __restrict__ rstd_in, int64_t rows, int64_t cols, Drop dp) {
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wpb = blockDim.x >> 6;
  constexpr bool FUSED = DADD || COLSUM;
  constexpr bool G_LDS = (FUSED || DY2) && CHUNKS == 4;
  constexpr bool G_PK = FUSED && CHUNKS == 1;
  constexpr bool G_F32 = !G_LDS && !G_PK;
  __shared__ __attribute__((aligned(16))) T g_lds[G_LDS ? CHUNKS * 512 : 8];
  float8 gw[G_F32 ? CHUNKS : 1], acc_dg[CHUNKS], acc_db[CHUNKS];
  uint4 gpk[G_PK ? CHUNKS : 1];
  float8 acc_cs[COLSUM ? CHUNKS : 1];
  if (G_LDS) {
    for (int64_t c = (int64_t)threadIdx.x * 8; c < cols;
         c += (int64_t)blockDim.x * 8)
      *reinterpret_cast<uint4*>(g_lds + c) =
          *reinterpret_cast<const uint4*>(gamma + c);
    __syncthreads();
  }
  auto gamma_at = [&](int k, int c) -> float8 {
    if (G_LDS) return load_bf16x8(g_lds + c);
    if (G_PK) {
      // opaque to the optimizer, or it hoists the unpack out of the row
      // loop and the eight fp32 registers are back
      asm volatile("" : "+v"(gpk[k].x), "+v"(gpk[k].y), "+v"(gpk[k].z),
                   "+v"(gpk[k].w));
      return load_bf16x8(reinterpret_cast<const T*>(&gpk[k]));
    }
    return gw[k];
  };
#pragma unroll
  for (int k = 0; k < CHUNKS; ++k) {
    const int c = (lane + k * 64) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      acc_dg[k].v[j] = 0.f;
      acc_db[k].v[j] = 0.f;
      if (COLSUM) acc_cs[k].v[j] = 0.f;
    }
    if (c < cols) {
      if (G_F32) gw[k] = load_bf16x8(gamma + c);
      if (G_PK) gpk[k] = *reinterpret_cast<const uint4*>(gamma + c);
    }
  }
  for (int64_t row = (int64_t)blockIdx.x * wpb + wid; row < rows;
       row += (int64_t)gridDim.x * wpb) {
    const int64_t base = row * cols;
    const float mean = mean_in[row];
    const float rstd = rstd_in[row];
    float sum_dyg = 0.f, sum_dygx = 0.f;
    float8 c_xhat[CACHE ? CHUNKS : 1], c_dy[CACHE ? CHUNKS : 1];
#pragma unroll
    for (int k = 0; k < CHUNKS; ++k) {
      const int c = (lane + k * 64) * 8;
      if (c >= cols) continue;
      float8 d = load_bf16x8(dy + base + c);
      if (DY2) {
        const float8 d2 = load_bf16x8(dy2 + base + c);
#pragma unroll
        for (int j = 0; j < 8; ++j) d.v[j] += d2.v[j];
      }
      const float8 f = load_bf16x8(s + base + c);
      const float8 g = gamma_at(k, c);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xhat = (f.v[j] - mean) * rstd;
        const float dyg = d.v[j] * g.v[j];
        if (CACHE) {
          c_xhat[k].v[j] = xhat;
          c_dy[k].v[j] = d.v[j];
        }
        sum_dyg += dyg;
        sum_dygx += dyg * xhat;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      sum_dyg += __shfl_down(sum_dyg, off, 64);
      sum_dygx += __shfl_down(sum_dygx, off, 64);
    }
    sum_dyg = __shfl(sum_dyg, 0, 64);
    sum_dygx = __shfl(sum_dygx, 0, 64);
    const float inv_cols = 1.f / cols;
#pragma unroll
    for (int k = 0; k < CHUNKS; ++k) {
      const int c = (lane + k * 64) * 8;
      if (c >= cols) continue;
      // drawn first and folded to one word, so that the philox state is
      // dead before the chunk's loads and gradient math need registers
      // (the column word is made opaque, or the compiler hoists the first
      // round's product of it out of the row loop: 2 VGPRs per chunk for
      // the whole kernel, spilled at CHUNKS = 4)
      int cc = c;
      asm volatile("" : "+v"(cc));
      const unsigned int km = keep_bytes(row, cc, dp).mask(dp.thresh);
      float8 dv, xh;
      if (CACHE) {
        dv = c_dy[k];
        xh = c_xhat[k];
      } else {
        // rows in flight fit L2: the re-reads hit cache
        float8 d = load_bf16x8(dy + base + c);
        if (DY2) {
          const float8 d2 = load_bf16x8(dy2 + base + c);
#pragma unroll
          for (int j = 0; j < 8; ++j) d.v[j] += d2.v[j];
        }
        const float8 f = load_bf16x8(s + base + c);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          dv.v[j] = d.v[j];
          xh.v[j] = (f.v[j] - mean) * rstd;
        }
      }
      const float8 g = gamma_at(k, c);
      float8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float dyg = dv.v[j] * g.v[j];
        o.v[j] = (dyg - (sum_dyg + xh.v[j] * sum_dygx) * inv_cols) * rstd;
        acc_dg[k].v[j] += dv.v[j] * xh.v[j];
        acc_db[k].v[j] += dv.v[j];
      }
      if (DADD) {
        const float8 a = load_bf16x8(dadd + base + c);
#pragma unroll
        for (int j = 0; j < 8; ++j) o.v[j] += a.v[j];
      }
      store_bf16x8(d_res + base + c, o);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        o.v[j] = ((km >> j) & 1u) ? o.v[j] * dp.inv_keep : 0.f;
        if (COLSUM) acc_cs[k].v[j] += o.v[j];
      }
      store_bf16x8(d_x + base + c, o);
    }
  }
  // Fold the block's four waves, outside the row loop, in wave order; the
  // block writes one partial row per plane (zeros from a wave with no row).
  constexpr int PLANES = COLSUM ? 3 : 2;
  constexpr int GROUP = CHUNKS <= 2 ? PLANES : 1;   // planes per barrier
  __shared__ __attribute__((aligned(16))) float red[3][GROUP][CHUNKS * 512];
  const int64_t prow = (int64_t)blockIdx.x * cols;
  auto post = [&](const float8 (&acc)[CHUNKS], int slot) {
    if (wid == 0) return;
#pragma unroll
    for (int k = 0; k < CHUNKS; ++k) {
      const int c = (lane + k * 64) * 8;
      if (c < cols) store_f32x8(&red[wid - 1][slot][c], acc[k]);
    }
  };
  auto fold = [&](float8 (&acc)[CHUNKS], int slot, float* part) {
    if (wid != 0) return;
#pragma unroll
    for (int k = 0; k < CHUNKS; ++k) {
      const int c = (lane + k * 64) * 8;
      if (c >= cols) continue;
      for (int w = 0; w < 3; ++w) {
        const float8 o = load_f32x8(&red[w][slot][c]);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[k].v[j] += o.v[j];
      }
      store_f32x8(part + prow + c, acc[k]);
    }
  };
  if constexpr (GROUP > 1) {
    post(acc_dg, 0);
    post(acc_db, 1);
    if constexpr (COLSUM) post(acc_cs, GROUP - 1);
    __syncthreads();
    fold(acc_dg, 0, dg_part);
    fold(acc_db, 1, db_part);
    if constexpr (COLSUM) fold(acc_cs, GROUP - 1, cs_part);
  } else {
    post(acc_dg, 0);
    __syncthreads();
    fold(acc_dg, 0, dg_part);
    __syncthreads();
    post(acc_db, 0);
    __syncthreads();
    fold(acc_db, 0, db_part);
    if constexpr (COLSUM) {
      __syncthreads();
      post(acc_cs, 0);
      __syncthreads();
      fold(acc_cs, 0, cs_part);
    }
  }
}

// The plain backward's fixed-order reduce of the partial rows (its kernel
// is private to its translation unit): blockIdx.y picks the plane, a block
// of 1024 threads covers 16 columns with 64 slices of the partial rows, a
// thread sums its slice in row order, 16 loads in flight, then the 64
// slice sums are added in slice order by one writer.  No float atomics;
// two calls give the same bits.  Outputs are stored as fp32 or as bf16.
struct DropRedPlane {
  void* out;            // [cols]
  const float* part;    // [nparts, cols]
  int bf16;
};
struct DropRedPlanes {
  DropRedPlane p[3];
};

constexpr int kRedCols = 16, kRedSlices = 64, kRedDepth = 16;

__global__ __launch_bounds__(kRedCols * kRedSlices) void
ln_dropout_rows_reduce_kernel(DropRedPlanes planes, int64_t nparts,
                              int64_t cols) {
  __shared__ float lds[kRedSlices][kRedCols];
  const DropRedPlane pl = planes.p[blockIdx.y];
  const int cx = threadIdx.x % kRedCols;
  const int sy = threadIdx.x / kRedCols;
  const int64_t c = (int64_t)blockIdx.x * kRedCols + cx;
  float sum = 0.f;
  if (c < cols) {
    for (int64_t p0 = sy; p0 < nparts; p0 += kRedSlices * kRedDepth) {
      float v[kRedDepth];
#pragma unroll
      for (int i = 0; i < kRedDepth; ++i) {
        const int64_t p = p0 + (int64_t)i * kRedSlices;
        v[i] = p < nparts ? pl.part[p * cols + c] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < kRedDepth; ++i) sum += v[i];
    }
  }
  lds[sy][cx] = sum;
  __syncthreads();
  if (sy == 0 && c < cols) {
    float t = lds[0][cx];
#pragma unroll
    for (int i = 1; i < kRedSlices; ++i) t += lds[i][cx];
    if (pl.bf16)
      reinterpret_cast<T*>(pl.out)[c] = (T)cvt_pk_bf16(t, t);
    else
      reinterpret_cast<float*>(pl.out)[c] = t;
  }
}

// ============================================================================
// out = D(x) (+ res) over [rows, cols]; the backward is the same kernel on
// the incoming gradient, dx = D(g).  Each thread owns ONE 8-column vector
// and strides by whole rows: the first rpp * vpr threads tile rpp
// consecutive rows, the few left over idle.  One 32-bit division at entry,
// no division or modulo in the loop.  The launcher guarantees rpp >= 1.
// ============================================================================
template <bool HAS_RES>
__global__ __launch_bounds__(256) void dropout_add_kernel(
    T* __restrict__ out, const T* __restrict__ x, const T* __restrict__ res,
    int64_t rows, int64_t cols, Drop dp) {
  const unsigned vpr = (unsigned)(cols / 8);
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned rpp = (gridDim.x * blockDim.x) / vpr;
  const unsigned r0 = g / vpr;
  if (r0 >= rpp) return;
  const int64_t c = (int64_t)(g - r0 * vpr) * 8;
  for (int64_t row = r0; row < rows; row += rpp) {
    const int64_t at = row * cols + c;
    float8 f = load_bf16x8(x + at);
    float8 r;
    if (HAS_RES) r = load_bf16x8(res + at);
    const KeepBytes kb = keep_bytes(row, c, dp);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float rv = HAS_RES ? r.v[j] : 0.f;
      f.v[j] = kb.keep(j, dp.thresh)
                   ? __builtin_fmaf(f.v[j], dp.inv_keep, rv)
                   : rv;
    }
    store_bf16x8(out + at, f);
  }
}

constexpr int kRowGrid = 4096;      // one-row-per-block forward
constexpr int kStreamGrid = 2048;   // 8 blocks of 256 threads per CU

int fwd_block(int64_t cols) {
  const int64_t need = cols / 8;    // float8 chunks in a row
  if (need <= 64) return 64;
  if (need <= 128) return 128;
  if (need <= 192) return 192;
  return 256;
}

int64_t bwd_parts(int64_t rows) {
  const int64_t wave_rows = (rows + 3) / 4;
  return wave_rows < 1024 ? (wave_rows > 0 ? wave_rows : 1) : 1024;
}

int dropout_add_grid(int64_t rows, int64_t cols) {
  const int64_t vpr = cols / 8;
  int64_t blocks = (rows * vpr + 255) / 256;
  if (blocks > kStreamGrid) blocks = kStreamGrid;
  // the kernel tiles whole rows: at least one row of threads
  const int64_t min_blocks = (vpr + 255) / 256;
  if (blocks < min_blocks) blocks = min_blocks;
  return (int)blocks;
}

Drop make_drop(uint64_t seed, int thresh, float inv_keep) {
  return {(unsigned int)seed, (unsigned int)(seed >> 32), thresh, inv_keep};
}

struct BwdArgs {
  T *d_x, *d_res;
  DropRedPlanes outs;
  const T *dy, *dy2, *s, *gamma, *dadd;
  const float *mean, *rstd;
  int64_t rows, cols;
  Drop dp;
  hipStream_t stream;
};

template <bool DADD, bool COLSUM, bool DY2>
void bwd_launch(const BwdArgs& a) {
  const int grid = (int)bwd_parts(a.rows);
  float* dg_part = const_cast<float*>(a.outs.p[0].part);
  float* db_part = const_cast<float*>(a.outs.p[1].part);
  float* cs_part = const_cast<float*>(a.outs.p[2].part);
#define EPL_LND_BWD(CH, CACHE)                                              \
  hipLaunchKernelGGL(                                                       \
      (layer_norm_dropout_bwd_kernel<CH, CACHE, DADD, COLSUM, DY2>),        \
      dim3(grid), dim3(256), 0, a.stream, a.d_x, a.d_res, dg_part, db_part, \
      cs_part, a.dy, a.dy2, a.s, a.gamma, a.dadd, a.mean, a.rstd, a.rows,   \
      a.cols, a.dp)
  if (a.cols <= 512)
    EPL_LND_BWD(1, true);
  else if (a.cols <= 1024)
    EPL_LND_BWD(2, true);
  else
    EPL_LND_BWD(4, false);
#undef EPL_LND_BWD
  hipLaunchKernelGGL(ln_dropout_rows_reduce_kernel,
                     dim3((unsigned)((a.cols + kRedCols - 1) / kRedCols),
                          COLSUM ? 3 : 2),
                     dim3(kRedCols * kRedSlices), 0, a.stream, a.outs,
                     (int64_t)grid, a.cols);
}

template <bool DADD, bool COLSUM>
void bwd_dy2(const BwdArgs& a) {
  if (a.dy2 != nullptr)
    bwd_launch<DADD, COLSUM, true>(a);
  else
    bwd_launch<DADD, COLSUM, false>(a);
}

}  // namespace

// extern "C" launchers (raw pointers + stream; bound to torch in
// bindings.hip, which checks every precondition named here)
extern "C" {

// bf16, cols % 8 == 0, cols <= 4096; res may be null, sum_out may not
void epl_layer_norm_dropout_fwd(void* out, const void* x, const void* res,
                                void* sum_out, const void* gamma,
                                const void* beta, float* mean, float* rstd,
                                int64_t rows, int64_t cols, float eps,
                                uint64_t seed, int thresh, float inv_keep,
                                hipStream_t stream) {
  const int grid = (int)(rows < kRowGrid ? rows : kRowGrid);
  const int block = fwd_block(cols);
  const bool two = cols > (int64_t)block * 8;
  const Drop dp = make_drop(seed, thresh, inv_keep);
#define EPL_LND_FWD(RES, CH)                                                \
  hipLaunchKernelGGL((layer_norm_dropout_fwd_kernel<RES, CH>), dim3(grid),  \
                     dim3(block), 0, stream, (T*)out, (const T*)x,          \
                     (const T*)res, (T*)sum_out, (const T*)gamma,           \
                     (const T*)beta, mean, rstd, rows, cols, eps, dp)
  if (res != nullptr) {
    if (two) EPL_LND_FWD(true, 2);
    else EPL_LND_FWD(true, 1);
  } else {
    if (two) EPL_LND_FWD(false, 2);
    else EPL_LND_FWD(false, 1);
  }
#undef EPL_LND_FWD
}

int64_t epl_layer_norm_dropout_bwd_parts(int64_t rows) {
  return bwd_parts(rows);
}

// bf16, cols % 8 == 0, cols <= 2048.  dadd / dy2 / colsum (with cs_part)
// may be null.  The partial planes hold epl_layer_norm_dropout_bwd_parts
// (rows) rows of cols floats each; *_bf16 say how dgamma, dbeta and colsum
// are stored.
void epl_layer_norm_dropout_bwd(void* d_x, void* d_res, void* dgamma,
                                void* dbeta, void* colsum, int g_bf16,
                                int b_bf16, int c_bf16, const void* dy,
                                const void* dy2, const void* s,
                                const void* gamma, const void* dadd,
                                const float* mean, const float* rstd,
                                float* dg_part, float* db_part,
                                float* cs_part, int64_t rows, int64_t cols,
                                uint64_t seed, int thresh, float inv_keep,
                                hipStream_t stream) {
  const bool has_cs = colsum != nullptr && cs_part != nullptr;
  BwdArgs a;
  a.d_x = (T*)d_x; a.d_res = (T*)d_res;
  a.outs.p[0] = {dgamma, dg_part, g_bf16};
  a.outs.p[1] = {dbeta, db_part, b_bf16};
  a.outs.p[2] = {has_cs ? colsum : nullptr, has_cs ? cs_part : nullptr,
                 c_bf16};
  a.dy = (const T*)dy; a.dy2 = (const T*)dy2; a.s = (const T*)s;
  a.gamma = (const T*)gamma; a.dadd = (const T*)dadd;
  a.mean = mean; a.rstd = rstd;
  a.rows = rows; a.cols = cols;
  a.dp = make_drop(seed, thresh, inv_keep);
  a.stream = stream;
  if (dadd != nullptr) {
    if (has_cs) bwd_dy2<true, true>(a);
    else bwd_dy2<true, false>(a);
  } else {
    if (has_cs) bwd_dy2<false, true>(a);
    else bwd_dy2<false, false>(a);
  }
}

// bf16 [rows, cols], cols % 8 == 0, cols / 8 < 2^21; res may be null.  The
// backward is the same call on the gradient with no res.
void epl_dropout_add(void* out, const void* x, const void* res, int64_t rows,
                     int64_t cols, uint64_t seed, int thresh, float inv_keep,
                     hipStream_t stream) {
  const int grid = dropout_add_grid(rows, cols);
  const Drop dp = make_drop(seed, thresh, inv_keep);
  if (res != nullptr)
    hipLaunchKernelGGL((dropout_add_kernel<true>), dim3(grid), dim3(256), 0,
                       stream, (T*)out, (const T*)x, (const T*)res, rows,
                       cols, dp);
  else
    hipLaunchKernelGGL((dropout_add_kernel<false>), dim3(grid), dim3(256), 0,
                       stream, (T*)out, (const T*)x, (const T*)res, rows,
                       cols, dp);
}

}  // extern "C"
