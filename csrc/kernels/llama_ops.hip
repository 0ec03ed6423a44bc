// LLaMA-block streaming kernels for gfx950: RMSNorm (optional fused residual
// add) forward / backward, in-place rotary position embedding on strided
// [B, S, N, D] views, and the SwiGLU gate on a packed [rows, 2F] GEMM
// output.  All bf16 in / out with 16-byte vector loads and stores, fp32
// arithmetic, every stored bf16 value rounded once by v_cvt_pk_bf16_f32.
// Column reductions go through per-block partial rows and a fixed-order
// second kernel: no float atomics anywhere, so two runs agree bitwise.
// Self-contained: the helpers below are this file's own.

#include <hip/hip_runtime.h>
#include <cstdint>

#define DEV __device__ __forceinline__

namespace {

using T = unsigned short;   // bf16 storage

struct float8 {
  float v[8];
};

using f32x2 = __attribute__((ext_vector_type(2))) float;
using bf16v2 = __attribute__((ext_vector_type(2))) __bf16;

// two floats -> packed bf16 pair in one v_cvt_pk_bf16_f32
DEV unsigned int cvt_pk_bf16(float a, float b) {
  f32x2 f = {a, b};
  return __builtin_bit_cast(unsigned int, __builtin_convertvector(f, bf16v2));
}

DEV float8 unpack_bf16x8(const uint4& raw) {
  float8 f;
  f.v[0] = __uint_as_float(raw.x << 16);
  f.v[1] = __uint_as_float(raw.x & 0xffff0000u);
  f.v[2] = __uint_as_float(raw.y << 16);
  f.v[3] = __uint_as_float(raw.y & 0xffff0000u);
  f.v[4] = __uint_as_float(raw.z << 16);
  f.v[5] = __uint_as_float(raw.z & 0xffff0000u);
  f.v[6] = __uint_as_float(raw.w << 16);
  f.v[7] = __uint_as_float(raw.w & 0xffff0000u);
  return f;
}

DEV uint4 load_raw8(const T* p) { return *reinterpret_cast<const uint4*>(p); }

DEV float8 load_bf16x8(const T* p) { return unpack_bf16x8(load_raw8(p)); }

DEV void store_bf16x8(T* p, const float8& f) {
  *reinterpret_cast<uint4*>(p) =
      make_uint4(cvt_pk_bf16(f.v[0], f.v[1]), cvt_pk_bf16(f.v[2], f.v[3]),
                 cvt_pk_bf16(f.v[4], f.v[5]), cvt_pk_bf16(f.v[6], f.v[7]));
}

DEV float8 load_f32x8(const float* p) {
  float8 f;
  const float4 a = *reinterpret_cast<const float4*>(p);
  const float4 b = *reinterpret_cast<const float4*>(p + 4);
  f.v[0] = a.x; f.v[1] = a.y; f.v[2] = a.z; f.v[3] = a.w;
  f.v[4] = b.x; f.v[5] = b.y; f.v[6] = b.z; f.v[7] = b.w;
  return f;
}

DEV void store_f32x8(float* p, const float8& f) {
  *reinterpret_cast<float4*>(p) = make_float4(f.v[0], f.v[1], f.v[2], f.v[3]);
  *reinterpret_cast<float4*>(p + 4) =
      make_float4(f.v[4], f.v[5], f.v[6], f.v[7]);
}

// butterfly sum: every lane ends with the same bits (a + b == b + a)
DEV float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Sum over the block's waves with ONE barrier: lane 0 of each wave posts
// its wave sum, every thread adds the (at most four) posts in wave order.
// lds holds two sets of four slots and the caller alternates `parity`
// from call to call: a set is rewritten two calls later, after a barrier
// every reader of it has passed.
DEV float block_sum(float v, float* lds, int parity) {
  v = wave_sum(v);
  const int nw = blockDim.x >> 6;
  if (nw == 1) return v;
  float* slot = lds + parity * 4;
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = slot[0];
  for (int w = 1; w < nw; ++w) t += slot[w];
  return t;
}

// ============================================================================
// RMSNorm forward: s = x (+ res); rstd = rsqrt(mean(s^2) + eps);
// out = s * rstd * gamma.  One row per block, the fp32 row cached in
// registers between the statistic and the scaling (HBM read once), gamma in
// registers across the block's rows.  CHUNKS = 8-column vectors per thread;
// the launcher picks the block so CHUNKS 1 / 2 / 4 covers cols <= 2048 /
// 4096 / 8192.  The addends of the one reduction are squares: nothing
// cancels, no pivot.  With HAS_RES the summed stream is written out too.
// ============================================================================
template <bool HAS_RES, int CHUNKS>
__global__ __launch_bounds__(256) void rms_norm_fwd_kernel(
    T* __restrict__ out, const T* __restrict__ x, const T* __restrict__ res,
    T* __restrict__ sum_out, const T* __restrict__ gamma,
    float* __restrict__ rstd_out, int64_t rows, int64_t cols, float eps) {
  __shared__ float lds[8];
  float8 cache[CHUNKS], gw[CHUNKS];
#pragma unroll
  for (int k = 0; k < CHUNKS; ++k) {
    const int64_t c = ((int64_t)threadIdx.x + k * blockDim.x) * 8;
    if (c < cols) gw[k] = load_bf16x8(gamma + c);
  }
  int parity = 0;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int64_t base = row * cols;
    float ssq = 0.f;
#pragma unroll
    for (int k = 0; k < CHUNKS; ++k) {
      const int64_t c = ((int64_t)threadIdx.x + k * blockDim.x) * 8;
      if (c >= cols) continue;
      float8 f = load_bf16x8(x + base + c);
      if (HAS_RES) {
        const float8 r = load_bf16x8(res + base + c);
#pragma unroll
        for (int j = 0; j < 8; ++j) f.v[j] += r.v[j];
        store_bf16x8(sum_out + base + c, f);
      }
      cache[k] = f;
#pragma unroll
      for (int j = 0; j < 8; ++j) ssq += f.v[j] * f.v[j];
    }
    ssq = block_sum(ssq, lds, parity);
    parity ^= 1;
    const float rstd = rsqrtf(ssq / cols + eps);
    if (threadIdx.x == 0) rstd_out[row] = rstd;
#pragma unroll
    for (int k = 0; k < CHUNKS; ++k) {
      const int64_t c = ((int64_t)threadIdx.x + k * blockDim.x) * 8;
      if (c >= cols) continue;
      float8 y;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        y.v[j] = cache[k].v[j] * rstd * gw[k].v[j];
      store_bf16x8(out + base + c, y);
    }
  }
}

// ============================================================================
// RMSNorm backward at the saved (s, rstd): xhat = s rstd,
//   dx = rstd (dy gamma - xhat mean(dy gamma xhat)) (+ dadd, fp32, before
//   the single rounding), dgamma = sum_rows dy xhat.
// A "team" owns a row: one wave (BLOCK = false, cols <= 2048, no barrier in
// the row loop) or the whole 256-thread block (BLOCK = true, cols <= 8192,
// one barrier per row).  Teams grid-stride over the rows.  The row's dy and
// s stay in registers as the packed bf16 they were loaded as (8 VGPRs per
// chunk) between the reduction and the dx pass; dgamma accumulates in
// registers over the team's rows and leaves as one partial row per block.
// ============================================================================
template <int CHUNKS, bool BLOCK, bool DADD>
__global__ __launch_bounds__(256) void rms_norm_bwd_kernel(
    T* __restrict__ dx, float* __restrict__ dg_part,
    const T* __restrict__ dy, const T* __restrict__ s,
    const T* __restrict__ gamma, const float* __restrict__ rstd_in,
    const T* __restrict__ dadd, int64_t rows, int64_t cols) {
  __shared__ float lds[8];
  constexpr int TW = BLOCK ? 256 : 64;             // team width
  const int tl = BLOCK ? (int)threadIdx.x : (int)(threadIdx.x & 63);
  const int64_t team = BLOCK ? (int64_t)blockIdx.x
                             : (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nteams = BLOCK ? (int64_t)gridDim.x : (int64_t)gridDim.x * 4;
  float8 gw[CHUNKS], acc[CHUNKS];
#pragma unroll
  for (int k = 0; k < CHUNKS; ++k) {
    const int64_t c = ((int64_t)tl + k * TW) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[k].v[j] = 0.f;
    if (c < cols) gw[k] = load_bf16x8(gamma + c);
  }
  const float inv_cols = 1.f / cols;
  int parity = 0;
  // BLOCK: `row` depends on blockIdx alone, so the block's threads make the
  // same number of trips and meet at the barrier inside block_sum
  for (int64_t row = team; row < rows; row += nteams) {
    const int64_t base = row * cols;
    const float rstd = rstd_in[row];
    uint4 rdy[CHUNKS], rs[CHUNKS];
    float b = 0.f;
#pragma unroll
    for (int k = 0; k < CHUNKS; ++k) {
      const int64_t c = ((int64_t)tl + k * TW) * 8;
      if (c >= cols) continue;
      rdy[k] = load_raw8(dy + base + c);
      rs[k] = load_raw8(s + base + c);
      const float8 d = unpack_bf16x8(rdy[k]);
      const float8 f = unpack_bf16x8(rs[k]);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        b += (d.v[j] * gw[k].v[j]) * (f.v[j] * rstd);
    }
    if (BLOCK) {
      b = block_sum(b, lds, parity);
      parity ^= 1;
    } else {
      b = wave_sum(b);
    }
    const float coef = b * inv_cols;
#pragma unroll
    for (int k = 0; k < CHUNKS; ++k) {
      const int64_t c = ((int64_t)tl + k * TW) * 8;
      if (c >= cols) continue;
      const float8 d = unpack_bf16x8(rdy[k]);
      const float8 f = unpack_bf16x8(rs[k]);
      float8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xhat = f.v[j] * rstd;
        o.v[j] = (d.v[j] * gw[k].v[j] - xhat * coef) * rstd;
        acc[k].v[j] += d.v[j] * xhat;
      }
      if (DADD) {
        const float8 a = load_bf16x8(dadd + base + c);
#pragma unroll
        for (int j = 0; j < 8; ++j) o.v[j] += a.v[j];
      }
      store_bf16x8(dx + base + c, o);
    }
  }
  // One partial row per BLOCK, zeros when it owned no row.  The wave form
  // folds its four waves first, outside the row loop: waves 1..3 post
  // their registers to LDS, wave 0 adds them in wave order.
  if constexpr (!BLOCK) {
    __shared__ __attribute__((aligned(16))) float red[3][CHUNKS * 512];
    const int wid = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < CHUNKS; ++k) {
      const int c = (tl + k * TW) * 8;
      if (wid > 0 && c < cols) store_f32x8(&red[wid - 1][c], acc[k]);
    }
    __syncthreads();
    if (wid > 0) return;
#pragma unroll
    for (int k = 0; k < CHUNKS; ++k) {
      const int c = (tl + k * TW) * 8;
      if (c >= cols) continue;
      for (int w = 0; w < 3; ++w) {
        const float8 o = load_f32x8(&red[w][c]);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[k].v[j] += o.v[j];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < CHUNKS; ++k) {
    const int64_t c = ((int64_t)tl + k * TW) * 8;
    if (c < cols)
      store_f32x8(dg_part + (int64_t)blockIdx.x * cols + c, acc[k]);
  }
}

// dgamma[c] = sum of the partial rows, in a fixed order: a block covers 16
// columns (64-byte row segments) with 16 slices of the partial rows, each
// slice summed in row order, then the 16 slice sums in slice order.
__global__ __launch_bounds__(256) void rms_dgamma_reduce_kernel(
    float* __restrict__ dgamma, const float* __restrict__ part,
    int64_t nparts, int64_t cols) {
  __shared__ float lds[16][16];
  const int cx = threadIdx.x & 15;
  const int sy = threadIdx.x >> 4;
  const int64_t c = (int64_t)blockIdx.x * 16 + cx;
  float sum = 0.f;
  if (c < cols)
    for (int64_t p = sy; p < nparts; p += 16) sum += part[p * cols + c];
  lds[sy][cx] = sum;
  __syncthreads();
  if (sy == 0 && c < cols) {
    float t = lds[0][cx];
#pragma unroll
    for (int i = 1; i < 16; ++i) t += lds[i][cx];
    dgamma[c] = t;
  }
}

// ============================================================================
// Rotary position embedding, in place, HF-LLaMA half-split convention:
// element i < D/2 of a head pairs with i + D/2,
//   y1 = x1 cos - x2 sin,  y2 = x2 cos + x1 sin,
// cos / sin from fp32 tables [L, D/2] at row pos0 + s.  `sign` = -1 applies
// the transpose (the inverse rotation, which is the backward).  x is a
// [B, S, N, D] view given by its element strides (last stride 1): the same
// kernel rotates the q and k slices of a packed [B, S, 3, H, D] buffer as
// N = 2H heads and never touches v, or a stand-alone q / k in either
// memory order.  A lane owns 8 consecutive i of both halves of one head
// and reads and writes exactly those 16 elements, so in place is race
// free.  No on-device trigonometry.
// ============================================================================
template <int D>
__global__ __launch_bounds__(256) void rope_kernel(
    T* __restrict__ x, const float* __restrict__ cos_t,
    const float* __restrict__ sin_t, int64_t sb, int64_t ss, int64_t sn,
    unsigned S, unsigned N, unsigned total, int64_t pos0, float sign) {
  constexpr int HALF = D / 2;
  constexpr int VPH = HALF / 8;                 // lanes per head: 4 or 8
  constexpr int LOG_VPH = VPH == 4 ? 2 : 3;
  // total < 2^31 and the grid holds at most 2^19 threads: no wrap
  for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < total;
       idx += gridDim.x * 256u) {
    const unsigned v = idx & (VPH - 1);
    const unsigned hn = idx >> LOG_VPH;
    const unsigned tok = hn / N;
    const unsigned n = hn - tok * N;
    const unsigned b = tok / S;
    const unsigned sq = tok - b * S;
    T* p = x + (int64_t)b * sb + (int64_t)sq * ss + (int64_t)n * sn + v * 8;
    const int64_t trow = (pos0 + sq) * HALF + v * 8;
    const float8 x1 = load_bf16x8(p);
    const float8 x2 = load_bf16x8(p + HALF);
    const float8 c = load_f32x8(cos_t + trow);
    const float8 sn8 = load_f32x8(sin_t + trow);
    float8 y1, y2;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float sj = sn8.v[j] * sign;          // exact
      y1.v[j] = x1.v[j] * c.v[j] - x2.v[j] * sj;
      y2.v[j] = x2.v[j] * c.v[j] + x1.v[j] * sj;
    }
    store_bf16x8(p, y1);
    store_bf16x8(p + HALF, y2);
  }
}

// ============================================================================
// SwiGLU on the packed [rows, 2F] output of one gate/up GEMM (gate =
// columns [0, F), up = [F, 2F)): out = silu(g) u.  The sigmoid is
// s = 1 / (1 + 2^(-g log2 e)): one v_exp_f32, one v_rcp_f32, no IEEE
// division; g = -100 overflows 2^w to inf and the reciprocal gives s = 0.
// Backward writes both halves of one [rows, 2F] gradient buffer:
//   dgate = dy u (s + g s (1 - s)),  dup = dy g s.
// Each thread owns ONE 8-column vector and strides by whole rows: the first
// rpp * vpr threads tile rpp consecutive rows, the few left over idle.  One
// 32-bit division at entry, none in the loop.  The launcher guarantees
// rpp >= 1.
// ============================================================================
DEV float sigmoid_lean(float g) {
  constexpr float c = (float)(-1.4426950408889634);
  const float e = __builtin_amdgcn_exp2f(g * c);
  return __builtin_amdgcn_rcpf(1.f + e);
}

__global__ __launch_bounds__(256) void swiglu_fwd_kernel(
    T* __restrict__ out, const T* __restrict__ gu, int64_t rows, int64_t f) {
  const unsigned vpr = (unsigned)(f / 8);
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned rpp = (gridDim.x * blockDim.x) / vpr;
  const unsigned r0 = g / vpr;
  if (r0 >= rpp) return;
  const int64_t c = (int64_t)(g - r0 * vpr) * 8;
  for (int64_t row = r0; row < rows; row += rpp) {
    const T* src = gu + row * 2 * f + c;
    const float8 gv = load_bf16x8(src);
    const float8 uv = load_bf16x8(src + f);
    float8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      o.v[j] = gv.v[j] * sigmoid_lean(gv.v[j]) * uv.v[j];
    store_bf16x8(out + row * f + c, o);
  }
}

__global__ __launch_bounds__(256) void swiglu_bwd_kernel(
    T* __restrict__ dgu, const T* __restrict__ dy, const T* __restrict__ gu,
    int64_t rows, int64_t f) {
  const unsigned vpr = (unsigned)(f / 8);
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned rpp = (gridDim.x * blockDim.x) / vpr;
  const unsigned r0 = g / vpr;
  if (r0 >= rpp) return;
  const int64_t c = (int64_t)(g - r0 * vpr) * 8;
  for (int64_t row = r0; row < rows; row += rpp) {
    const int64_t at = row * 2 * f + c;
    const float8 gv = load_bf16x8(gu + at);
    const float8 uv = load_bf16x8(gu + at + f);
    const float8 d = load_bf16x8(dy + row * f + c);
    float8 dg, du;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float sg = sigmoid_lean(gv.v[j]);
      const float gs = gv.v[j] * sg;
      dg.v[j] = (d.v[j] * uv.v[j]) * (sg + gs * (1.f - sg));
      du.v[j] = (d.v[j] * gv.v[j]) * sg;
    }
    store_bf16x8(dgu + at, dg);
    store_bf16x8(dgu + at + f, du);
  }
}

constexpr int kStreamGrid = 2048;   // 8 blocks of 256 threads per CU
constexpr int kRowGrid = 4096;      // one-row-per-block forward
constexpr int kBwdGrid = 1024;      // backward blocks = partial-row budget

int rms_fwd_block(int64_t cols) {
  const int64_t need = cols / 8;
  if (need <= 64) return 64;
  if (need <= 128) return 128;
  if (need <= 192) return 192;
  return 256;
}

template <bool HAS_RES>
void rms_fwd_launch(T* out, const T* x, const T* res, T* sum_out,
                    const T* gamma, float* rstd, int64_t rows, int64_t cols,
                    float eps, hipStream_t stream) {
  const int grid = (int)(rows < kRowGrid ? rows : kRowGrid);
  const int block = rms_fwd_block(cols);
  if (cols <= 2048)
    hipLaunchKernelGGL((rms_norm_fwd_kernel<HAS_RES, 1>), dim3(grid),
                       dim3(block), 0, stream, out, x, res, sum_out, gamma,
                       rstd, rows, cols, eps);
  else if (cols <= 4096)
    hipLaunchKernelGGL((rms_norm_fwd_kernel<HAS_RES, 2>), dim3(grid),
                       dim3(256), 0, stream, out, x, res, sum_out, gamma,
                       rstd, rows, cols, eps);
  else
    hipLaunchKernelGGL((rms_norm_fwd_kernel<HAS_RES, 4>), dim3(grid),
                       dim3(256), 0, stream, out, x, res, sum_out, gamma,
                       rstd, rows, cols, eps);
}

template <bool DADD>
void rms_bwd_launch(T* dx, float* dg_part, const T* dy, const T* s,
                    const T* gamma, const float* rstd, const T* dadd,
                    int grid, int64_t rows, int64_t cols,
                    hipStream_t stream) {
#define EPL_RMS_BWD(CH, BLK)                                               \
  hipLaunchKernelGGL((rms_norm_bwd_kernel<CH, BLK, DADD>), dim3(grid),     \
                     dim3(256), 0, stream, dx, dg_part, dy, s, gamma, rstd, \
                     dadd, rows, cols)
  if (cols <= 512)
    EPL_RMS_BWD(1, false);
  else if (cols <= 1024)
    EPL_RMS_BWD(2, false);
  else if (cols <= 2048)
    EPL_RMS_BWD(4, false);
  else if (cols <= 4096)
    EPL_RMS_BWD(2, true);
  else
    EPL_RMS_BWD(4, true);
#undef EPL_RMS_BWD
}

// blocks of the backward launch; one wave (cols <= 2048) or one block per row
int rms_bwd_grid(int64_t rows, int64_t cols) {
  const int64_t want = cols <= 2048 ? (rows + 3) / 4 : rows;
  return (int)(want < kBwdGrid ? (want > 0 ? want : 1) : kBwdGrid);
}

int swiglu_grid(int64_t rows, int64_t f) {
  const int64_t vpr = f / 8;
  int64_t blocks = (rows * vpr + 255) / 256;
  if (blocks > kStreamGrid) blocks = kStreamGrid;
  // the kernels tile whole rows: at least one row of threads
  const int64_t min_blocks = (vpr + 255) / 256;
  if (blocks < min_blocks) blocks = min_blocks;
  return (int)blocks;
}

}  // namespace

// extern "C" launchers (raw pointers + stream; bound to torch in
// bindings.hip, which checks every precondition named here)
extern "C" {

// bf16, cols % 8 == 0, 8 <= cols <= 8192, rows >= 1
void epl_rms_norm_fwd(void* out, const void* x, const void* res,
                      void* sum_out, const void* gamma, float* rstd,
                      int64_t rows, int64_t cols, float eps,
                      hipStream_t stream) {
  if (res != nullptr)
    rms_fwd_launch<true>((T*)out, (const T*)x, (const T*)res, (T*)sum_out,
                         (const T*)gamma, rstd, rows, cols, eps, stream);
  else
    rms_fwd_launch<false>((T*)out, (const T*)x, nullptr, nullptr,
                          (const T*)gamma, rstd, rows, cols, eps, stream);
}

// partial rows the backward writes: dg_part holds this many rows of cols
int64_t epl_rms_norm_bwd_parts(int64_t rows, int64_t cols) {
  return (int64_t)rms_bwd_grid(rows, cols);
}

void epl_rms_norm_bwd(void* dx, float* dgamma, const void* dy, const void* s,
                      const void* gamma, const float* rstd, const void* dadd,
                      float* dg_part, int64_t rows, int64_t cols,
                      hipStream_t stream) {
  const int grid = rms_bwd_grid(rows, cols);
  if (dadd != nullptr)
    rms_bwd_launch<true>((T*)dx, dg_part, (const T*)dy, (const T*)s,
                         (const T*)gamma, rstd, (const T*)dadd, grid, rows,
                         cols, stream);
  else
    rms_bwd_launch<false>((T*)dx, dg_part, (const T*)dy, (const T*)s,
                          (const T*)gamma, rstd, nullptr, grid, rows, cols,
                          stream);
  hipLaunchKernelGGL(rms_dgamma_reduce_kernel,
                     dim3((unsigned)((cols + 15) / 16)), dim3(256), 0, stream,
                     dgamma, dg_part, epl_rms_norm_bwd_parts(rows, cols),
                     cols);
}

// x: [B, S, N, D] view by element strides, D in (64, 128), last stride 1;
// B * S * N * D / 16 < 2^31; tables hold at least pos0 + S rows of D / 2
void epl_rope(void* x, const float* cos_t, const float* sin_t, int64_t sb,
              int64_t ss, int64_t sn, int64_t b, int64_t s, int64_t n,
              int64_t d, int64_t pos0, bool inverse, hipStream_t stream) {
  const int64_t total = b * s * n * (d / 16);
  if (total == 0) return;
  int64_t blocks = (total + 255) / 256;
  if (blocks > kStreamGrid) blocks = kStreamGrid;
  const float sign = inverse ? -1.f : 1.f;
  if (d == 64)
    hipLaunchKernelGGL(rope_kernel<64>, dim3((unsigned)blocks), dim3(256), 0,
                       stream, (T*)x, cos_t, sin_t, sb, ss, sn, (unsigned)s,
                       (unsigned)n, (unsigned)total, pos0, sign);
  else
    hipLaunchKernelGGL(rope_kernel<128>, dim3((unsigned)blocks), dim3(256), 0,
                       stream, (T*)x, cos_t, sin_t, sb, ss, sn, (unsigned)s,
                       (unsigned)n, (unsigned)total, pos0, sign);
}

// bf16, f % 8 == 0, rows >= 1
void epl_swiglu_fwd(void* out, const void* gu, int64_t rows, int64_t f,
                    hipStream_t stream) {
  hipLaunchKernelGGL(swiglu_fwd_kernel, dim3(swiglu_grid(rows, f)), dim3(256),
                     0, stream, (T*)out, (const T*)gu, rows, f);
}

void epl_swiglu_bwd(void* dgu, const void* dy, const void* gu, int64_t rows,
                    int64_t f, hipStream_t stream) {
  hipLaunchKernelGGL(swiglu_bwd_kernel, dim3(swiglu_grid(rows, f)), dim3(256),
                     0, stream, (T*)dgu, (const T*)dy, (const T*)gu, rows, f);
}

}  // extern "C"
