// Hand-written CDNA4 (gfx950) kernels for the MI355X-native parallel library.
//
// These replace the hot-path ops the reference leaves to TF (the reference's
// native layer, /root/reference/csrc/, contains no device kernels at all —
// only NCCL glue).  Everything here is memory-bound streaming work, designed
// per the CDNA4 rules: 256-thread blocks (4 waves of 64), bf16 loaded as
// packed ushort vectors (8-16 B/lane), fp32 accumulation, grid-stride loops
// capped near 2048 blocks so the 256-CU chip is filled without launch spam,
// LDS used for per-block column-reduction partials (dgamma/dbeta/dbias) so
// global atomics fire once per block, not once per row.
//
// Optimizer kernels operate on FLAT ARENAS: the Python engine concatenates
// every parameter of a taskgraph into one contiguous buffer (master fp32 /
// model bf16 / grad), so one AdamW step is ONE kernel over one flat stream —
// no multi-tensor metadata tables, no per-parameter launches.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdint>
#include <cmath>

#define DEV __device__ __forceinline__

namespace {

constexpr int kBlock = 256;
constexpr int kMaxGrid = 4096;  // >> 256 CUs; grid-stride covers the rest

DEV float bf2f(unsigned short u) {
  unsigned int x = (unsigned int)u << 16;
  return __uint_as_float(x);
}

using f32x2 = __attribute__((ext_vector_type(2))) float;
using bf16v2 = __attribute__((ext_vector_type(2))) __bf16;

// two floats -> packed bf16 pair in one v_cvt_pk_bf16_f32: round to
// nearest even, and a NaN stays a NaN
DEV unsigned int cvt_pk_bf16(float a, float b) {
  f32x2 f = {a, b};
  return __builtin_bit_cast(unsigned int, __builtin_convertvector(f, bf16v2));
}

DEV unsigned short f2bf(float f) {
  // the hardware convert, not the integer rounding add x + 0x7fff + lsb:
  // that add carries a NaN with a full high mantissa half into +-0 or Inf
  return (unsigned short)cvt_pk_bf16(f, f);
}

struct ushort8 {
  unsigned short v[8];
};
struct float8 {
  float v[8];
};

DEV float8 load_bf16x8(const unsigned short* p) {
  const ushort8 raw = *reinterpret_cast<const ushort8*>(p);
  float8 f;
#pragma unroll
  for (int i = 0; i < 8; ++i) f.v[i] = bf2f(raw.v[i]);
  return f;
}

DEV void store_bf16x8(unsigned short* p, const float8& f) {
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

inline int grid_for(int64_t work_items) {
  int64_t blocks = (work_items + kBlock - 1) / kBlock;
  return (int)(blocks < kMaxGrid ? (blocks > 0 ? blocks : 1) : kMaxGrid);
}

// 1 / (1 - beta^step) of the fp32 beta the kernels use, in double and
// rounded once: in fp32 the subtraction amplifies powf's rounding by
// beta^step / (1 - beta^step), about 100 ulp at beta 0.999 and steps 2-5
inline float inv_bias_correction(float beta, int step) {
  return (float)(1.0 / (1.0 - std::pow((double)beta, (double)step)));
}

// ---- block-wide reduction (256 threads = 4 waves) ---------------------------
DEV float block_reduce_sum(float val, float* lds /* >= 4 floats */) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    val += __shfl_down(val, off, 64);
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int nwaves = blockDim.x >> 6;
  if (lane == 0) lds[wave] = val;
  __syncthreads();
  if (wave == 0) {
    val = lane < nwaves ? lds[lane] : 0.f;
#pragma unroll
    for (int off = 2; off > 0; off >>= 1)
      val += __shfl_down(val, off, 64);
    if (lane == 0) lds[0] = val;
  }
  __syncthreads();
  return lds[0];
}

DEV float block_reduce_max(float val, float* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    val = fmaxf(val, __shfl_down(val, off, 64));
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int nwaves = blockDim.x >> 6;
  if (lane == 0) lds[wave] = val;
  __syncthreads();
  if (wave == 0) {
    val = lane < nwaves ? lds[lane] : -INFINITY;
#pragma unroll
    for (int off = 2; off > 0; off >>= 1)
      val = fmaxf(val, __shfl_down(val, off, 64));
    if (lane == 0) lds[0] = val;
  }
  __syncthreads();
  return lds[0];
}

// ============================================================================
// Fused AdamW over a flat arena.
//   master: fp32 "true" parameters (flat).
//   param : optional bf16 working copy written back after the update.
//   grad  : bf16 or fp32 gradients; multiplied by inv_scale (AMP unscale
//           fused in).  Decoupled weight decay (AdamW).
// ============================================================================
template <bool GRAD_BF16, bool HAS_BF16_PARAM>
__global__ void fused_adamw_kernel(
    float* __restrict__ master, unsigned short* __restrict__ param,
    const void* __restrict__ grad_raw, float* __restrict__ m,
    float* __restrict__ v, int64_t n, float lr, float beta1, float beta2,
    float eps, float weight_decay, float inv_bias1, float inv_bias2,
    float inv_scale) {
  const int64_t nvec = n / 8;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t base = i * 8;
    float8 g;
    if (GRAD_BF16)
      g = load_bf16x8(
          reinterpret_cast<const unsigned short*>(grad_raw) + base);
    else
      g = load_f32x8(reinterpret_cast<const float*>(grad_raw) + base);
    float8 pm = load_f32x8(master + base);
    float8 mm = load_f32x8(m + base);
    float8 vv = load_f32x8(v + base);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float gk = g.v[k] * inv_scale;
      float mk = beta1 * mm.v[k] + (1.f - beta1) * gk;
      float vk = beta2 * vv.v[k] + (1.f - beta2) * gk * gk;
      float mhat = mk * inv_bias1;
      float vhat = vk * inv_bias2;
      float pk = pm.v[k];
      pk -= lr * (mhat / (sqrtf(vhat) + eps) + weight_decay * pk);
      mm.v[k] = mk;
      vv.v[k] = vk;
      pm.v[k] = pk;
    }
    store_f32x8(m + base, mm);
    store_f32x8(v + base, vv);
    store_f32x8(master + base, pm);
    if (HAS_BF16_PARAM) store_bf16x8(param + base, pm);
  }
  // scalar tail
  const int64_t tail = nvec * 8;
  for (int64_t i = tail + blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float gk = (GRAD_BF16
                    ? bf2f(reinterpret_cast<const unsigned short*>(grad_raw)[i])
                    : reinterpret_cast<const float*>(grad_raw)[i]) *
               inv_scale;
    float mk = beta1 * m[i] + (1.f - beta1) * gk;
    float vk = beta2 * v[i] + (1.f - beta2) * gk * gk;
    float pk = master[i];
    pk -= lr * ((mk * inv_bias1) / (sqrtf(vk * inv_bias2) + eps) +
                weight_decay * pk);
    m[i] = mk;
    v[i] = vk;
    master[i] = pk;
    if (HAS_BF16_PARAM) param[i] = f2bf(pk);
  }
}

// ============================================================================
// Fused LAMB over a flat arena, phase kernels.
//   Phase 1: update m, v; write the raw Adam update u into a scratch buffer;
//            accumulate per-CHUNK squared norms of (param, update) so the
//            Python side can compute per-parameter trust ratios (chunks are
//            parameter boundaries in the flat arena).
//   Phase 2: p -= lr * ratio[chunk] * (u + wd*p) applied per chunk.
// Chunk ids come from a per-8-element chunk-index map built once on the host.
// ============================================================================
__global__ void lamb_phase1_kernel(
    const float* __restrict__ master, const void* __restrict__ grad_raw,
    bool grad_bf16, float* __restrict__ m, float* __restrict__ v,
    float* __restrict__ update, const int* __restrict__ chunk_of,
    float* __restrict__ wnorm_sq, float* __restrict__ unorm_sq, int64_t n,
    float beta1, float beta2, float eps, float weight_decay, float inv_bias1,
    float inv_bias2, float inv_scale) {
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float gk = (grad_bf16
                    ? bf2f(reinterpret_cast<const unsigned short*>(grad_raw)[i])
                    : reinterpret_cast<const float*>(grad_raw)[i]) *
               inv_scale;
    float mk = beta1 * m[i] + (1.f - beta1) * gk;
    float vk = beta2 * v[i] + (1.f - beta2) * gk * gk;
    m[i] = mk;
    v[i] = vk;
    float pk = master[i];
    float u = (mk * inv_bias1) / (sqrtf(vk * inv_bias2) + eps) +
              weight_decay * pk;
    update[i] = u;
    const int c = chunk_of[i >> 3];
    atomicAdd(&wnorm_sq[c], pk * pk);
    atomicAdd(&unorm_sq[c], u * u);
  }
}

__global__ void lamb_phase2_kernel(float* __restrict__ master,
                                   unsigned short* __restrict__ param,
                                   const float* __restrict__ update,
                                   const int* __restrict__ chunk_of,
                                   const float* __restrict__ ratio, int64_t n,
                                   float lr) {
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int c = chunk_of[i >> 3];
    float pk = master[i] - lr * ratio[c] * update[i];
    master[i] = pk;
    if (param != nullptr) param[i] = f2bf(pk);
  }
}

// ============================================================================
// LayerNorm forward with optional fused residual add: s = x (+ res);
// y = (s - mean(s)) * rstd(s) * gamma + beta.  One block per row.  The
// bf16 fast path caches each thread's own row values in REGISTERS between
// the statistics pass and the normalize pass (threads re-touch the same
// columns), so HBM is read once and LDS carries only the 8-float block
// reduction.  CHUNKS = row float8-chunks per thread; the launcher picks
// the block size so CHUNKS <= 2 covers cols <= 4096 at 256 threads.
// With HAS_RES the summed input s is also written out (the tensor the
// backward normalizes against and, for pre-LN blocks, the residual
// stream).  Saves mean and rstd.
// Statistics in two passes over the cached row: mean = p + sum(s - p) / n
// around a pivot p, then var = sum((s - mean)^2) / n.  (sumsq / n - mean^2
// cancels in fp32 on rows with an offset: NaN on near-constant rows.)
// ============================================================================
template <bool HAS_RES, int CHUNKS>
__global__ void layer_norm_fwd_bf16_kernel(
    void* __restrict__ out, const void* __restrict__ x,
    const void* __restrict__ res, void* __restrict__ sum_out,
    const void* __restrict__ gamma, const void* __restrict__ beta,
    float* __restrict__ mean_out, float* __restrict__ rstd_out, int64_t rows,
    int64_t cols, float eps) {
  __shared__ float lds[8];
  using T = unsigned short;
  float8 cache[CHUNKS];
  float8 gw[CHUNKS], bw[CHUNKS];
#pragma unroll
  for (int k = 0; k < CHUNKS; ++k) {
    const int64_t c = ((int64_t)threadIdx.x + k * blockDim.x) * 8;
    if (c < cols) {
      gw[k] = load_bf16x8(reinterpret_cast<const T*>(gamma) + c);
      bw[k] = load_bf16x8(reinterpret_cast<const T*>(beta) + c);
    }
  }
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int64_t base = row * cols;
    // pivot: the row's first element, read by every thread (one broadcast
    // load).  Summing s - pivot keeps the fp32 error of the mean
    // proportional to the row's spread, not to its offset.
    float piv = bf2f(reinterpret_cast<const T*>(x)[base]);
    if (HAS_RES) piv += bf2f(reinterpret_cast<const T*>(res)[base]);
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < CHUNKS; ++k) {
      const int64_t c = ((int64_t)threadIdx.x + k * blockDim.x) * 8;
      if (c >= cols) continue;
      float8 f = load_bf16x8(reinterpret_cast<const T*>(x) + base + c);
      if (HAS_RES) {
        float8 r = load_bf16x8(reinterpret_cast<const T*>(res) + base + c);
#pragma unroll
        for (int j = 0; j < 8; ++j) f.v[j] += r.v[j];
        store_bf16x8(reinterpret_cast<T*>(sum_out) + base + c, f);
      }
      cache[k] = f;
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += f.v[j] - piv;
    }
    sum = block_reduce_sum(sum, lds);
    const float mean = piv + sum / cols;
    // variance as the mean of squared deviations from that mean, out of
    // the cached row: all addends are >= 0, nothing cancels
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
      store_bf16x8(reinterpret_cast<T*>(out) + base + c, y);
    }
    __syncthreads();
  }
}

// generic (fp32 / large-cols) forward: re-reads the row for the variance
// and for the normalize pass
template <bool BF16, bool HAS_RES>
__global__ void layer_norm_fwd_kernel(
    void* __restrict__ out, const void* __restrict__ x,
    const void* __restrict__ res, void* __restrict__ sum_out,
    const void* __restrict__ gamma, const void* __restrict__ beta,
    float* __restrict__ mean_out, float* __restrict__ rstd_out, int64_t rows,
    int64_t cols, float eps) {
  __shared__ float lds[8];
  using T = unsigned short;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int64_t base = row * cols;
    // s = x (+ res) in fp32, before any rounding of the stored sum
    auto s_at = [&](int64_t i) -> float {
      float fv = BF16 ? bf2f(reinterpret_cast<const T*>(x)[i])
                      : reinterpret_cast<const float*>(x)[i];
      if (HAS_RES)
        fv += BF16 ? bf2f(reinterpret_cast<const T*>(res)[i])
                   : reinterpret_cast<const float*>(res)[i];
      return fv;
    };
    const float piv = s_at(base);   // pivot, as in the fast kernel
    float sum = 0.f;
    for (int64_t c = threadIdx.x; c < cols; c += blockDim.x) {
      const float fv = s_at(base + c);
      if (HAS_RES) {
        if (BF16)
          reinterpret_cast<T*>(sum_out)[base + c] = f2bf(fv);
        else
          reinterpret_cast<float*>(sum_out)[base + c] = fv;
      }
      sum += fv - piv;
    }
    sum = block_reduce_sum(sum, lds);
    const float mean = piv + sum / cols;
    // second read of the row (L2-resident) for the squared deviations: a
    // shifted two-moment form would still cancel when the pivot is the
    // row's outlier
    float ssq = 0.f;
    for (int64_t c = threadIdx.x; c < cols; c += blockDim.x) {
      const float d = s_at(base + c) - mean;
      ssq += d * d;
    }
    __syncthreads();
    ssq = block_reduce_sum(ssq, lds);
    const float rstd = rsqrtf(ssq / cols + eps);
    if (threadIdx.x == 0) {
      mean_out[row] = mean;
      rstd_out[row] = rstd;
    }
    const void* nin = HAS_RES ? sum_out : x;
    for (int64_t c = threadIdx.x; c < cols; c += blockDim.x) {
      float fv = BF16 ? bf2f(reinterpret_cast<const T*>(nin)[base + c])
                      : reinterpret_cast<const float*>(nin)[base + c];
      float gv = BF16 ? bf2f(reinterpret_cast<const T*>(gamma)[c])
                      : reinterpret_cast<const float*>(gamma)[c];
      float bv = BF16 ? bf2f(reinterpret_cast<const T*>(beta)[c])
                      : reinterpret_cast<const float*>(beta)[c];
      float y = (fv - mean) * rstd * gv + bv;
      if (BF16)
        reinterpret_cast<T*>(out)[base + c] = f2bf(y);
      else
        reinterpret_cast<float*>(out)[base + c] = y;
    }
    __syncthreads();
  }
}

// bf16 fast backward: ONE ROW PER WAVE — no barrier in the row loop.  Each
// wave reduces its row with shuffles, keeps the row image in registers between
// the reduction and the dx pass (HBM read-once/write-once; CHUNKS=4
// re-reads the row from L2 instead), accumulates dgamma/dbeta in
// registers across its rows.  After the row loop the block's four waves
// fold their accumulators through LDS in wave order and the block writes
// ONE partial row per plane — no atomics here; partial_rows_reduce_kernel
// sums the partial rows in a fixed order.  CHUNKS = ceil(cols/8/64),
// cols <= 2048.
//   DADD   : dx += dadd (bf16 [rows, cols]) in fp32 before the single
//            bf16 rounding — the gradient arriving through the summed
//            stream of a fused-residual LN.
//   COLSUM : a third accumulator, the column sum of the fp32 value that
//            is rounded into dx (DADD included), written to cs_part —
//            the bias gradient of the Linear that produced x.
//   DY2    : a second upstream gradient (bf16 [rows, cols]): dy = dy + dy2
//            in fp32 right after the loads, never rounded to bf16 — the
//            two consumers of a post-LN output, without autograd's add
//            kernel in between.
// With all flags off the row loop is the two-plane kernel's.
// The waves-per-SIMD bound pins each CHUNKS to the occupancy its plain
// form reaches (5 / 3 / 3); to fit the extra plane under it the fused
// forms stop holding gamma as fp32 registers where those are short:
// CHUNKS=1 keeps it packed bf16 (4 VGPRs, unpacked at each use), CHUNKS=4
// (there also the plain form with DY2) stages it once per block in LDS
// (4 KB).
template <int CHUNKS, bool CACHE, bool DADD, bool COLSUM, bool DY2>
__global__ __launch_bounds__(256, CHUNKS == 1 ? 5 : 3) void
layer_norm_bwd_bf16_kernel(
    void* __restrict__ dx, float* __restrict__ dg_part,
    float* __restrict__ db_part, float* __restrict__ cs_part,
    const void* __restrict__ dy, const void* __restrict__ dy2,
    const void* __restrict__ x,
    const void* __restrict__ gamma, const void* __restrict__ dadd,
    const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
    int64_t rows, int64_t cols) {
  using T = unsigned short;
  const int lane = threadIdx.x & 63;
  // wave in block (0..3), as a scalar: the row, its base offset and its
  // mean / rstd then live in SGPRs and the loads address scalar base +
  // lane offset
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wpb = blockDim.x >> 6;                // waves per block
  constexpr bool FUSED = DADD || COLSUM;
  constexpr bool G_LDS = (FUSED || DY2) && CHUNKS == 4;  // gamma from LDS
  constexpr bool G_PK = FUSED && CHUNKS == 1;     // gamma packed in VGPRs
  constexpr bool G_F32 = !G_LDS && !G_PK;
  __shared__ __attribute__((aligned(16))) T g_lds[G_LDS ? CHUNKS * 512 : 8];
  float8 gw[G_F32 ? CHUNKS : 1], acc_dg[CHUNKS], acc_db[CHUNKS];
  uint4 gpk[G_PK ? CHUNKS : 1];
  float8 acc_cs[COLSUM ? CHUNKS : 1];
  if (G_LDS) {
    for (int64_t c = (int64_t)threadIdx.x * 8; c < cols;
         c += (int64_t)blockDim.x * 8)
      *reinterpret_cast<uint4*>(g_lds + c) =
          *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(gamma) +
                                          c);
    __syncthreads();
  }
  // gamma of chunk k (columns c .. c+7) as fp32
  auto gamma_at = [&](int k, int64_t c) -> float8 {
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
    const int64_t c = ((int64_t)lane + k * 64) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      acc_dg[k].v[j] = 0.f;
      acc_db[k].v[j] = 0.f;
      if (COLSUM) acc_cs[k].v[j] = 0.f;
    }
    if (c < cols) {
      if (G_F32)
        gw[k] = load_bf16x8(reinterpret_cast<const T*>(gamma) + c);
      if (G_PK)
        gpk[k] = *reinterpret_cast<const uint4*>(
            reinterpret_cast<const T*>(gamma) + c);
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
      const int64_t c = ((int64_t)lane + k * 64) * 8;
      if (c >= cols) continue;
      float8 d = load_bf16x8(reinterpret_cast<const T*>(dy) + base + c);
      if (DY2) {
        const float8 d2 =
            load_bf16x8(reinterpret_cast<const T*>(dy2) + base + c);
#pragma unroll
        for (int j = 0; j < 8; ++j) d.v[j] += d2.v[j];
      }
      float8 f = load_bf16x8(reinterpret_cast<const T*>(x) + base + c);
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
      const int64_t c = ((int64_t)lane + k * 64) * 8;
      if (c >= cols) continue;
      float8 dv, xh;
      if (CACHE) {
        dv = c_dy[k];
        xh = c_xhat[k];
      } else {
        // rows in flight fit L2: the re-reads hit cache
        float8 d = load_bf16x8(reinterpret_cast<const T*>(dy) + base + c);
        if (DY2) {
          const float8 d2 =
              load_bf16x8(reinterpret_cast<const T*>(dy2) + base + c);
#pragma unroll
          for (int j = 0; j < 8; ++j) d.v[j] += d2.v[j];
        }
        float8 f = load_bf16x8(reinterpret_cast<const T*>(x) + base + c);
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
        const float8 a =
            load_bf16x8(reinterpret_cast<const T*>(dadd) + base + c);
#pragma unroll
        for (int j = 0; j < 8; ++j) o.v[j] += a.v[j];
      }
      if (COLSUM) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc_cs[k].v[j] += o.v[j];
      }
      store_bf16x8(reinterpret_cast<T*>(dx) + base + c, o);
    }
  }
  // Fold the block's four waves, outside the row loop: waves 1..3 post
  // their accumulators to LDS, wave 0 adds them in wave order and writes
  // the block's partial row (zeros from a wave that owned no row).
  // CHUNKS <= 2 posts every plane at once (one barrier; 36 KB at most, so
  // the blocks of a CU still fit their waves-per-SIMD bound in 160 KB);
  // CHUNKS = 4 posts a plane at a time through one 24 KB buffer.
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

// How the reducers below leave a column's sum: added to the fp32 value
// that is there (the pre-zeroed outputs of the older bindings), or stored
// as fp32 / as bf16 (one packed-convert rounding) over whatever was there.
enum : int { kRedAccF32 = 0, kRedStoreF32 = 1, kRedStoreBF16 = 2 };

struct RedPlane {
  void* out;            // [cols]
  const float* part;    // [nparts, cols]
  int mode;
};
struct RedPlanes {
  RedPlane p[3];
};

// out[c] (op)= sum of the partial rows of column c, in a fixed order and
// by one writer: blockIdx.y picks the plane, a block of 1024 threads covers
// 16 columns (64-byte row segments) with 64 slices of the partial rows.  A
// thread sums its slice in row order, 16 loads in flight at a time (at
// 1024 partial rows every load of the kernel is issued before the first
// add: the kernel is latency bound, not bandwidth bound), then the 64
// slice sums are added in slice order.  No float atomics; two calls give
// the same bits.
constexpr int kRedCols = 16, kRedSlices = 64, kRedDepth = 16;

__global__ __launch_bounds__(kRedCols * kRedSlices) void
partial_rows_reduce_kernel(RedPlanes planes, int64_t nparts, int64_t cols) {
  __shared__ float lds[kRedSlices][kRedCols];
  const RedPlane pl = planes.p[blockIdx.y];
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
    if (pl.mode == kRedStoreBF16)
      reinterpret_cast<unsigned short*>(pl.out)[c] = f2bf(t);
    else if (pl.mode == kRedStoreF32)
      reinterpret_cast<float*>(pl.out)[c] = t;
    else
      reinterpret_cast<float*>(pl.out)[c] += t;
  }
}

// generic (fp32 / large-cols) backward: LDS partials + global re-read
template <bool BF16>
__global__ void layer_norm_bwd_kernel(
    void* __restrict__ dx, float* __restrict__ dgamma,
    float* __restrict__ dbeta, const void* __restrict__ dy,
    const void* __restrict__ x, const void* __restrict__ gamma,
    const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
    int64_t rows, int64_t cols) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* part_dg = reinterpret_cast<float*>(smem);            // [cols]
  float* part_db = part_dg + cols;                            // [cols]
  __shared__ float lds[8];
  using T = unsigned short;
  for (int64_t c = threadIdx.x; c < cols; c += blockDim.x) {
    part_dg[c] = 0.f;
    part_db[c] = 0.f;
  }
  __syncthreads();
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int64_t base = row * cols;
    const float mean = mean_in[row];
    const float rstd = rstd_in[row];
    float sum_dyg = 0.f, sum_dygx = 0.f;
    for (int64_t c = threadIdx.x; c < cols; c += blockDim.x) {
      const float dv = BF16 ? bf2f(reinterpret_cast<const T*>(dy)[base + c])
                            : reinterpret_cast<const float*>(dy)[base + c];
      const float fv = BF16 ? bf2f(reinterpret_cast<const T*>(x)[base + c])
                            : reinterpret_cast<const float*>(x)[base + c];
      const float gv = BF16 ? bf2f(reinterpret_cast<const T*>(gamma)[c])
                            : reinterpret_cast<const float*>(gamma)[c];
      const float xhat = (fv - mean) * rstd;
      const float dyg = dv * gv;
      sum_dyg += dyg;
      sum_dygx += dyg * xhat;
      part_dg[c] += dv * xhat;
      part_db[c] += dv;
    }
    __syncthreads();
    sum_dyg = block_reduce_sum(sum_dyg, lds);
    __syncthreads();
    sum_dygx = block_reduce_sum(sum_dygx, lds);
    const float inv_cols = 1.f / cols;
    for (int64_t c = threadIdx.x; c < cols; c += blockDim.x) {
      const float dv = BF16 ? bf2f(reinterpret_cast<const T*>(dy)[base + c])
                            : reinterpret_cast<const float*>(dy)[base + c];
      const float fv = BF16 ? bf2f(reinterpret_cast<const T*>(x)[base + c])
                            : reinterpret_cast<const float*>(x)[base + c];
      const float gv = BF16 ? bf2f(reinterpret_cast<const T*>(gamma)[c])
                            : reinterpret_cast<const float*>(gamma)[c];
      const float xhat = (fv - mean) * rstd;
      const float o = (dv * gv - (sum_dyg + xhat * sum_dygx) * inv_cols) *
                      rstd;
      if (BF16)
        reinterpret_cast<T*>(dx)[base + c] = f2bf(o);
      else
        reinterpret_cast<float*>(dx)[base + c] = o;
    }
    __syncthreads();
  }
  for (int64_t c = threadIdx.x; c < cols; c += blockDim.x) {
    atomicAdd(&dgamma[c], part_dg[c]);
    atomicAdd(&dbeta[c], part_db[c]);
  }
}

// ============================================================================
// Fused bias + GeLU (tanh approximation), forward and backward.
// ============================================================================
DEV float fast_tanh(float u) {
  // tanh(u) = 1 - 2/(e^2u + 1): one fast exp instead of tanhf's polynomial
  // + range-reduction chain (bf16-accurate; numerics-tested vs torch)
  return 1.f - 2.f / (__expf(2.f * u) + 1.f);
}

DEV float gelu_f(float x) {
  const float k0 = 0.7978845608028654f;   // sqrt(2/pi)
  const float k1 = 0.044715f;
  return 0.5f * x * (1.f + fast_tanh(k0 * (x + k1 * x * x * x)));
}

DEV float gelu_grad_f(float x) {
  const float k0 = 0.7978845608028654f;
  const float k1 = 0.044715f;
  const float t = fast_tanh(k0 * (x + k1 * x * x * x));
  const float dt = (1.f - t * t) * k0 * (1.f + 3.f * k1 * x * x);
  return 0.5f * (1.f + t) + 0.5f * x * dt;
}

// ---- bf16 paths: lean arithmetic -------------------------------------------
// With u = k0 (x + k1 x^3):  0.5 (1 + tanh u) = 1 / (1 + e^{-2u}) =: s, so
//   gelu(x)  = x s
//   gelu'(x) = s + x s (1 - s) (2 k0 + 6 k0 k1 x^2)
// e^{-2u} is ONE v_exp_f32 (exp2 with -2 k0 log2(e) folded into the cubic)
// and s ONE v_rcp_f32 — no IEEE division, no tanh.  Both are ~1 ulp fp32,
// far inside the bf16 rounding of the result.  x -> -inf side: e = +inf,
// s = 0; x -> +inf side: e = 0, s = 1.
DEV float gelu_sigmoid(float x) {
  constexpr float c0 = (float)(-2.0 * 0.7978845608028654 *
                               1.4426950408889634);  // -2 sqrt(2/pi) log2(e)
  constexpr float c1 = (float)(-2.0 * 0.7978845608028654 *
                               1.4426950408889634 * 0.044715);
  const float e = __builtin_amdgcn_exp2f(x * (c0 + c1 * x * x));
  return __builtin_amdgcn_rcpf(1.f + e);
}

DEV float gelu_lean(float x) { return x * gelu_sigmoid(x); }

DEV float gelu_grad_lean(float x) {
  constexpr float d0 = (float)(2.0 * 0.7978845608028654);  // 2 sqrt(2/pi)
  constexpr float d1 = (float)(6.0 * 0.7978845608028654 * 0.044715);
  const float s = gelu_sigmoid(x);
  return s + x * s * (1.f - s) * (d0 + d1 * x * x);
}

DEV void store_bf16x8_pk(unsigned short* p, const float8& f) {
  *reinterpret_cast<uint4*>(p) =
      make_uint4(cvt_pk_bf16(f.v[0], f.v[1]), cvt_pk_bf16(f.v[2], f.v[3]),
                 cvt_pk_bf16(f.v[4], f.v[5]), cvt_pk_bf16(f.v[6], f.v[7]));
}

template <bool BF16>
__global__ void bias_gelu_fwd_kernel(void* __restrict__ out,
                                     const void* __restrict__ x,
                                     const void* __restrict__ bias,
                                     int64_t rows, int64_t cols) {
  using T = unsigned short;
  const int64_t n = rows * cols;
  if (BF16) {
    // Each thread owns ONE 8-column vector and strides by whole rows, so
    // its bias stays in registers and the loop has no modulo: the first
    // rpp * vpr threads tile rpp consecutive rows (flat, coalesced), the
    // few left over idle.  The launcher guarantees rpp >= 1.
    const unsigned vpr = (unsigned)(cols / 8);            // vectors per row
    const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned rpp = (gridDim.x * blockDim.x) / vpr;  // rows per pass
    const unsigned r0 = g / vpr;
    if (r0 >= rpp) return;
    const int64_t c = (int64_t)(g - r0 * vpr) * 8;
    const float8 b = load_bf16x8(reinterpret_cast<const T*>(bias) + c);
    for (int64_t row = r0; row < rows; row += rpp) {
      const int64_t base = row * cols + c;
      float8 f = load_bf16x8(reinterpret_cast<const T*>(x) + base);
      float8 o;
#pragma unroll
      for (int k = 0; k < 8; ++k) o.v[k] = gelu_lean(f.v[k] + b.v[k]);
      store_bf16x8_pk(reinterpret_cast<T*>(out) + base, o);
    }
  } else {
    for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
      const float xv = reinterpret_cast<const float*>(x)[i] +
                       reinterpret_cast<const float*>(bias)[i % cols];
      reinterpret_cast<float*>(out)[i] = gelu_f(xv);
    }
  }
}

// bf16 fast path: one row-segment per wave, dbias accumulated in
// registers across rows and flushed to per-wave partial rows.  SEGS = row
// segments of 512 columns; each wave owns one 512-col segment across ALL
// rows so its dbias registers cover exactly its columns.  Wave w owns
// segment w % segs and writes partial row w of [nwaves][512], which is
// row w / segs of a row-major [nwaves / segs, cols] matrix: the layout
// partial_rows_reduce_kernel sums, in a fixed order and without atomics.
__global__ void bias_gelu_bwd_bf16_kernel(
    void* __restrict__ dx, float* __restrict__ db_part,
    const void* __restrict__ dy, const void* __restrict__ x,
    const void* __restrict__ bias, int64_t rows, int64_t cols) {
  using T = unsigned short;
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  const int64_t segs = cols / 512;              // cols % 512 == 0
  float8 acc;
#pragma unroll
  for (int j = 0; j < 8; ++j) acc.v[j] = 0.f;
  const int64_t wave_id = (int64_t)blockIdx.x * wpb + wid;
  const int64_t nwaves = (int64_t)gridDim.x * wpb;
  // walk (row, my fixed segment) pairs: wave w owns segment w % segs
  const int64_t myseg = wave_id % segs;
  const int64_t c0 = myseg * 512 + (int64_t)lane * 8;
  const int64_t step = nwaves / segs;
  float8 bw = load_bf16x8(reinterpret_cast<const T*>(bias) + c0);
  for (int64_t row = wave_id / segs; row < rows; row += step) {
    const int64_t base = row * cols + c0;
    float8 d = load_bf16x8(reinterpret_cast<const T*>(dy) + base);
    float8 f = load_bf16x8(reinterpret_cast<const T*>(x) + base);
    float8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float g = d.v[j] * gelu_grad_lean(f.v[j] + bw.v[j]);
      o.v[j] = g;
      acc.v[j] += g;
    }
    store_bf16x8_pk(reinterpret_cast<T*>(dx) + base, o);
  }
  store_f32x8(db_part + wave_id * 512 + (int64_t)lane * 8, acc);
}

template <bool BF16>
__global__ void bias_gelu_bwd_kernel(void* __restrict__ dx,
                                     float* __restrict__ dbias,
                                     const void* __restrict__ dy,
                                     const void* __restrict__ x,
                                     const void* __restrict__ bias,
                                     int64_t rows, int64_t cols) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* part_db = reinterpret_cast<float*>(smem);  // [cols]
  using T = unsigned short;
  for (int64_t c = threadIdx.x; c < cols; c += blockDim.x) part_db[c] = 0.f;
  __syncthreads();
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int64_t base = row * cols;
    if (BF16) {
      for (int64_t c = threadIdx.x * 8; c < cols; c += (int64_t)blockDim.x * 8) {
        float8 d = load_bf16x8(reinterpret_cast<const T*>(dy) + base + c);
        float8 f = load_bf16x8(reinterpret_cast<const T*>(x) + base + c);
        float8 b = load_bf16x8(reinterpret_cast<const T*>(bias) + c);
        float8 o;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float g = d.v[k] * gelu_grad_f(f.v[k] + b.v[k]);
          o.v[k] = g;
          part_db[c + k] += g;
        }
        store_bf16x8(reinterpret_cast<T*>(dx) + base + c, o);
      }
    } else {
      for (int64_t c = threadIdx.x; c < cols; c += blockDim.x) {
        const float g = reinterpret_cast<const float*>(dy)[base + c] *
                        gelu_grad_f(reinterpret_cast<const float*>(x)[base + c] +
                                    reinterpret_cast<const float*>(bias)[c]);
        reinterpret_cast<float*>(dx)[base + c] = g;
        part_db[c] += g;
      }
    }
  }
  __syncthreads();
  for (int64_t c = threadIdx.x; c < cols; c += blockDim.x)
    atomicAdd(&dbias[c], part_db[c]);
}

// ============================================================================
// Fused softmax cross-entropy over (possibly vocab-sharded) logits.
// Forward: per row, max + sum(exp) in one pass each; writes per-row
// (max, sumexp, loss-contribution).  For the TP-sharded case the Python side
// allreduces max/sumexp between the two phases (reference semantics:
// /root/reference/epl/ops/distributed_losses.py:58-109).
//   Phase A (local): row max and sum exp(x - rowmax), plus the local logit at
//   the target (if the target falls in this shard's [vocab_begin, end)).
//   Phase B (local, after reduction): dlogits = softmax - onehot.
// ============================================================================
template <bool BF16>
__global__ void ce_rowstats_kernel(const void* __restrict__ logits,
                                   const int64_t* __restrict__ targets,
                                   float* __restrict__ row_max,
                                   float* __restrict__ row_sumexp,
                                   float* __restrict__ target_logit,
                                   int64_t rows, int64_t cols,
                                   int64_t vocab_begin, int64_t ignore_index,
                                   bool skip_ignored) {
  __shared__ float lds[8];
  using T = unsigned short;
  const bool vec = BF16 && (cols % 8 == 0);
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int64_t base = row * cols;
    // skip_ignored: a row the loss ignores is not read (uniform over the
    // block); it gets the statistics of a neutral row, max 0 and sum 1, so
    // log(sum) + max = 0 and a cross-shard rescale exp(max - gmax) is 1
    if (skip_ignored && targets[row] == ignore_index) {
      if (threadIdx.x == 0) {
        row_max[row] = 0.f;
        row_sumexp[row] = 1.f;
        target_logit[row] = 0.f;
      }
      continue;
    }
    float vmax = -INFINITY;
    if (vec) {
      const T* lr = reinterpret_cast<const T*>(logits) + base;
      for (int64_t c = threadIdx.x * 8; c < cols;
           c += (int64_t)blockDim.x * 8) {
        float8 f = load_bf16x8(lr + c);
#pragma unroll
        for (int k = 0; k < 8; ++k) vmax = fmaxf(vmax, f.v[k]);
      }
    } else {
      for (int64_t c = threadIdx.x; c < cols; c += blockDim.x) {
        const float v = BF16
            ? bf2f(reinterpret_cast<const T*>(logits)[base + c])
            : reinterpret_cast<const float*>(logits)[base + c];
        vmax = fmaxf(vmax, v);
      }
    }
    vmax = block_reduce_max(vmax, lds);
    __syncthreads();
    float sum = 0.f;
    if (vec) {
      const T* lr = reinterpret_cast<const T*>(logits) + base;
      for (int64_t c = threadIdx.x * 8; c < cols;
           c += (int64_t)blockDim.x * 8) {
        float8 f = load_bf16x8(lr + c);
#pragma unroll
        for (int k = 0; k < 8; ++k) sum += expf(f.v[k] - vmax);
      }
    } else {
      for (int64_t c = threadIdx.x; c < cols; c += blockDim.x) {
        const float v = BF16
            ? bf2f(reinterpret_cast<const T*>(logits)[base + c])
            : reinterpret_cast<const float*>(logits)[base + c];
        sum += expf(v - vmax);
      }
    }
    sum = block_reduce_sum(sum, lds);
    if (threadIdx.x == 0) {
      row_max[row] = vmax;
      // raw sum at this shard's max; Python rescales by
      // exp(local_max - global_max) before summing across shards.
      row_sumexp[row] = sum;
      const int64_t tgt = targets[row];
      float tl = 0.f;
      if (tgt != ignore_index && tgt >= vocab_begin &&
          tgt < vocab_begin + cols) {
        const int64_t c = tgt - vocab_begin;
        tl = BF16 ? bf2f(reinterpret_cast<const T*>(logits)[base + c])
                  : reinterpret_cast<const float*>(logits)[base + c];
      }
      target_logit[row] = tl;
    }
    __syncthreads();
  }
}

template <bool BF16>
__global__ void ce_backward_kernel(void* __restrict__ dlogits,
                                   const void* __restrict__ logits,
                                   const int64_t* __restrict__ targets,
                                   const float* __restrict__ gmax,
                                   const float* __restrict__ gsumexp,
                                   const float* __restrict__ dloss,
                                   int64_t rows, int64_t cols,
                                   int64_t vocab_begin, int64_t ignore_index,
                                   float scale) {
  using T = unsigned short;
  const bool vec = BF16 && (cols % 8 == 0);
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int64_t base = row * cols;
    const int64_t tgt = targets[row];
    if (tgt == ignore_index) {
      // a row of +0 without reading its logits or statistics (uniform
      // over the block): g * 0 would be NaN where those are not finite
      if (vec) {
        T* dr = reinterpret_cast<T*>(dlogits) + base;
        for (int64_t c = threadIdx.x * 8; c < cols;
             c += (int64_t)blockDim.x * 8)
          *reinterpret_cast<uint4*>(dr + c) = make_uint4(0u, 0u, 0u, 0u);
      } else {
        for (int64_t c = threadIdx.x; c < cols; c += blockDim.x) {
          if (BF16)
            reinterpret_cast<T*>(dlogits)[base + c] = 0;
          else
            reinterpret_cast<float*>(dlogits)[base + c] = 0.f;
        }
      }
      continue;
    }
    const float m = gmax[row];
    const float inv_sum = 1.f / gsumexp[row];
    const float dl = dloss[row] * scale;
    const int64_t tc = tgt - vocab_begin;
    if (vec) {
      const T* lr = reinterpret_cast<const T*>(logits) + base;
      T* dr = reinterpret_cast<T*>(dlogits) + base;
      for (int64_t c = threadIdx.x * 8; c < cols;
           c += (int64_t)blockDim.x * 8) {
        float8 f = load_bf16x8(lr + c);
        float8 o;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          float g = expf(f.v[k] - m) * inv_sum;
          if (tc == c + k) g -= 1.f;
          o.v[k] = g * dl;
        }
        store_bf16x8(dr + c, o);
      }
    } else {
      for (int64_t c = threadIdx.x; c < cols; c += blockDim.x) {
        const float v = BF16
            ? bf2f(reinterpret_cast<const T*>(logits)[base + c])
            : reinterpret_cast<const float*>(logits)[base + c];
        float g = expf(v - m) * inv_sum;
        if (tc == c) g -= 1.f;
        g *= dl;
        if (BF16)
          reinterpret_cast<T*>(dlogits)[base + c] = f2bf(g);
        else
          reinterpret_cast<float*>(dlogits)[base + c] = g;
      }
    }
  }
}

// ============================================================================
// Flat-arena utilities: zero / scale / axpy / casts / sq-norm.
// ============================================================================
__global__ void scale_f32_kernel(float* __restrict__ p, int64_t n, float s) {
  const int64_t nvec = n / 4;
  float4* p4 = reinterpret_cast<float4*>(p);
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += (int64_t)gridDim.x * blockDim.x) {
    float4 v = p4[i];
    v.x *= s; v.y *= s; v.z *= s; v.w *= s;
    p4[i] = v;
  }
  for (int64_t i = nvec * 4 + blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    p[i] *= s;
}

__global__ void scale_bf16_kernel(unsigned short* __restrict__ p, int64_t n,
                                  float s) {
  const int64_t nvec = n / 8;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += (int64_t)gridDim.x * blockDim.x) {
    float8 v = load_bf16x8(p + i * 8);
#pragma unroll
    for (int k = 0; k < 8; ++k) v.v[k] *= s;
    store_bf16x8(p + i * 8, v);
  }
  for (int64_t i = nvec * 8 + blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    p[i] = f2bf(bf2f(p[i]) * s);
}

__global__ void f32_to_bf16_kernel(unsigned short* __restrict__ dst,
                                   const float* __restrict__ src, int64_t n) {
  const int64_t nvec = n / 8;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += (int64_t)gridDim.x * blockDim.x)
    store_bf16x8(dst + i * 8, load_f32x8(src + i * 8));
  for (int64_t i = nvec * 8 + blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    dst[i] = f2bf(src[i]);
}

__global__ void bf16_to_f32_kernel(float* __restrict__ dst,
                                   const unsigned short* __restrict__ src,
                                   int64_t n) {
  const int64_t nvec = n / 8;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += (int64_t)gridDim.x * blockDim.x)
    store_f32x8(dst + i * 8, load_bf16x8(src + i * 8));
  for (int64_t i = nvec * 8 + blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    dst[i] = bf2f(src[i]);
}

template <bool BF16>
__global__ void sqnorm_kernel(const void* __restrict__ p, int64_t n,
                              float* __restrict__ out) {
  __shared__ float lds[8];
  using T = unsigned short;
  float acc = 0.f;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float v = BF16 ? bf2f(reinterpret_cast<const T*>(p)[i])
                         : reinterpret_cast<const float*>(p)[i];
    acc += v * v;
  }
  acc = block_reduce_sum(acc, lds);
  if (threadIdx.x == 0) atomicAdd(out, acc);
}

}  // namespace

// ============================================================================

// ============================================================================
// Column sum (Linear bias gradient): db[c] = sum_r dy[r, c].
// torch's generic reduce runs at ~2.2 TB/s on [65536, 1024] bf16; this
// pair streams bf16x8 rows into fp32 stripe partials (no atomics in the
// hot pass, same pattern as the LN backward) and a tiny reduce kernel
// folds the stripes.  ~73 of these per BERT-Large step (qkv/proj/fc2
// biases).
// ============================================================================
template <bool BF16>
__global__ void colsum_partial_kernel(const void* __restrict__ dy,
                                      float* __restrict__ partial,
                                      int64_t rows, int64_t cols,
                                      int64_t stripes) {
  // grid: (ceil(cols/(256*8)), stripes); each thread owns 8 columns
  const int64_t c = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (c >= cols) return;
  const int64_t per = (rows + stripes - 1) / stripes;
  const int64_t r0 = (int64_t)blockIdx.y * per;
  const int64_t r1 = r0 + per < rows ? r0 + per : rows;
  float8 acc = {};
  for (int64_t r = r0; r < r1; ++r) {
    if (BF16) {
      const float8 v =
          load_bf16x8(reinterpret_cast<const unsigned short*>(dy) +
                      r * cols + c);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc.v[k] += v.v[k];
    } else {
      const float* p = reinterpret_cast<const float*>(dy) + r * cols + c;
#pragma unroll
      for (int k = 0; k < 8; ++k) acc.v[k] += p[k];
    }
  }
  store_f32x8(partial + (int64_t)blockIdx.y * cols + c, acc);
}

template <bool BF16>
__global__ void colsum_reduce_kernel(void* __restrict__ db,
                                     const float* __restrict__ partial,
                                     int64_t stripes, int64_t cols) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cols) return;
  float s = 0.f;
  for (int64_t p = 0; p < stripes; ++p) s += partial[p * cols + c];
  if (BF16)
    reinterpret_cast<unsigned short*>(db)[c] = f2bf(s);
  else
    reinterpret_cast<float*>(db)[c] = s;
}

// blocks of the LN fast backward = partial rows per plane
inline int64_t ln_bwd_parts(int64_t rows) {
  const int64_t wave_rows = (rows + 3) / 4;
  return wave_rows < 1024 ? (wave_rows > 0 ? wave_rows : 1) : 1024;
}

struct LnBwdArgs {
  void* dx;
  RedPlanes outs;        // dgamma, dbeta, colsum with their partial planes
  const void *dy, *dy2, *x, *gamma, *dadd;
  const float *mean, *rstd;
  int64_t rows, cols;
  hipStream_t stream;
};

// LN fast backward + fixed-order reduce for one flag combination
template <bool DADD, bool COLSUM, bool DY2>
static void ln_bwd_fast_launch(const LnBwdArgs& a) {
  const int grid = (int)ln_bwd_parts(a.rows);
  float* dg_part = const_cast<float*>(a.outs.p[0].part);
  float* db_part = const_cast<float*>(a.outs.p[1].part);
  float* cs_part = const_cast<float*>(a.outs.p[2].part);
  if (a.cols <= 512)
    hipLaunchKernelGGL(
        (layer_norm_bwd_bf16_kernel<1, true, DADD, COLSUM, DY2>), dim3(grid),
        dim3(256), 0, a.stream, a.dx, dg_part, db_part, cs_part, a.dy, a.dy2,
        a.x, a.gamma, a.dadd, a.mean, a.rstd, a.rows, a.cols);
  else if (a.cols <= 1024)
    hipLaunchKernelGGL(
        (layer_norm_bwd_bf16_kernel<2, true, DADD, COLSUM, DY2>), dim3(grid),
        dim3(256), 0, a.stream, a.dx, dg_part, db_part, cs_part, a.dy, a.dy2,
        a.x, a.gamma, a.dadd, a.mean, a.rstd, a.rows, a.cols);
  else
    hipLaunchKernelGGL(
        (layer_norm_bwd_bf16_kernel<4, false, DADD, COLSUM, DY2>), dim3(grid),
        dim3(256), 0, a.stream, a.dx, dg_part, db_part, cs_part, a.dy, a.dy2,
        a.x, a.gamma, a.dadd, a.mean, a.rstd, a.rows, a.cols);
  hipLaunchKernelGGL(partial_rows_reduce_kernel,
                     dim3((unsigned)((a.cols + kRedCols - 1) / kRedCols),
                          COLSUM ? 3 : 2),
                     dim3(kRedCols * kRedSlices), 0, a.stream, a.outs, (int64_t)grid, a.cols);
}

template <bool DADD, bool COLSUM>
static void ln_bwd_fast_dy2(const LnBwdArgs& a) {
  if (a.dy2 != nullptr)
    ln_bwd_fast_launch<DADD, COLSUM, true>(a);
  else
    ln_bwd_fast_launch<DADD, COLSUM, false>(a);
}

// extern "C" launchers (raw pointers + stream; bound to torch in bindings.hip)
// ============================================================================
extern "C" {

void epl_fused_adamw(float* master, unsigned short* param_bf16,
                     const void* grad, bool grad_bf16, float* m, float* v,
                     int64_t n, float lr, float beta1, float beta2, float eps,
                     float weight_decay, int step, float inv_scale,
                     hipStream_t stream) {
  const float inv_bias1 = inv_bias_correction(beta1, step);
  const float inv_bias2 = inv_bias_correction(beta2, step);
  const int grid = grid_for((n + 7) / 8);
  if (grad_bf16) {
    if (param_bf16)
      hipLaunchKernelGGL((fused_adamw_kernel<true, true>), dim3(grid),
                         dim3(kBlock), 0, stream, master, param_bf16, grad, m,
                         v, n, lr, beta1, beta2, eps, weight_decay, inv_bias1,
                         inv_bias2, inv_scale);
    else
      hipLaunchKernelGGL((fused_adamw_kernel<true, false>), dim3(grid),
                         dim3(kBlock), 0, stream, master, param_bf16, grad, m,
                         v, n, lr, beta1, beta2, eps, weight_decay, inv_bias1,
                         inv_bias2, inv_scale);
  } else {
    if (param_bf16)
      hipLaunchKernelGGL((fused_adamw_kernel<false, true>), dim3(grid),
                         dim3(kBlock), 0, stream, master, param_bf16, grad, m,
                         v, n, lr, beta1, beta2, eps, weight_decay, inv_bias1,
                         inv_bias2, inv_scale);
    else
      hipLaunchKernelGGL((fused_adamw_kernel<false, false>), dim3(grid),
                         dim3(kBlock), 0, stream, master, param_bf16, grad, m,
                         v, n, lr, beta1, beta2, eps, weight_decay, inv_bias1,
                         inv_bias2, inv_scale);
  }
}

void epl_lamb_phase1(const float* master, const void* grad, bool grad_bf16,
                     float* m, float* v, float* update, const int* chunk_of,
                     float* wnorm_sq, float* unorm_sq, int64_t n, float beta1,
                     float beta2, float eps, float weight_decay, int step,
                     float inv_scale, hipStream_t stream) {
  const float inv_bias1 = inv_bias_correction(beta1, step);
  const float inv_bias2 = inv_bias_correction(beta2, step);
  const int grid = grid_for(n);
  hipLaunchKernelGGL(lamb_phase1_kernel, dim3(grid), dim3(kBlock), 0, stream,
                     master, grad, grad_bf16, m, v, update, chunk_of, wnorm_sq,
                     unorm_sq, n, beta1, beta2, eps, weight_decay, inv_bias1,
                     inv_bias2, inv_scale);
}

void epl_lamb_phase2(float* master, unsigned short* param_bf16,
                     const float* update, const int* chunk_of,
                     const float* ratio, int64_t n, float lr,
                     hipStream_t stream) {
  const int grid = grid_for(n);
  hipLaunchKernelGGL(lamb_phase2_kernel, dim3(grid), dim3(kBlock), 0, stream,
                     master, param_bf16, update, chunk_of, ratio, n, lr);
}

static int ln_block_for(int64_t cols) {
  // maximize threads per row: CHUNKS=1 whenever cols/8 fits in <=256
  // threads; CHUNKS=2 only for cols in (2048, 4096]
  int64_t need = (cols + 7) / 8;          // float8 chunks in a row
  if (need <= 64) return 64;
  if (need <= 128) return 128;
  if (need <= 192) return 192;
  return 256;
}

void epl_layer_norm_fwd(void* out, const void* x, const void* res,
                        void* sum_out, const void* gamma, const void* beta,
                        float* mean, float* rstd, int64_t rows, int64_t cols,
                        float eps, bool bf16, hipStream_t stream) {
  const int grid = (int)(rows < kMaxGrid ? rows : kMaxGrid);
  const bool has_res = res != nullptr;
  if (bf16 && cols % 8 == 0 && cols <= 2 * 256 * 8) {
    const int block = ln_block_for(cols);
    const bool two = cols > (int64_t)block * 8;
    if (has_res) {
      if (two)
        hipLaunchKernelGGL((layer_norm_fwd_bf16_kernel<true, 2>), dim3(grid),
                           dim3(block), 0, stream, out, x, res, sum_out,
                           gamma, beta, mean, rstd, rows, cols, eps);
      else
        hipLaunchKernelGGL((layer_norm_fwd_bf16_kernel<true, 1>), dim3(grid),
                           dim3(block), 0, stream, out, x, res, sum_out,
                           gamma, beta, mean, rstd, rows, cols, eps);
    } else {
      if (two)
        hipLaunchKernelGGL((layer_norm_fwd_bf16_kernel<false, 2>), dim3(grid),
                           dim3(block), 0, stream, out, x, res, sum_out,
                           gamma, beta, mean, rstd, rows, cols, eps);
      else
        hipLaunchKernelGGL((layer_norm_fwd_bf16_kernel<false, 1>), dim3(grid),
                           dim3(block), 0, stream, out, x, res, sum_out,
                           gamma, beta, mean, rstd, rows, cols, eps);
    }
    return;
  }
  if (bf16) {
    if (has_res)
      hipLaunchKernelGGL((layer_norm_fwd_kernel<true, true>), dim3(grid),
                         dim3(kBlock), 0, stream, out, x, res, sum_out,
                         gamma, beta, mean, rstd, rows, cols, eps);
    else
      hipLaunchKernelGGL((layer_norm_fwd_kernel<true, false>), dim3(grid),
                         dim3(kBlock), 0, stream, out, x, res, sum_out,
                         gamma, beta, mean, rstd, rows, cols, eps);
  } else {
    if (has_res)
      hipLaunchKernelGGL((layer_norm_fwd_kernel<false, true>), dim3(grid),
                         dim3(kBlock), 0, stream, out, x, res, sum_out,
                         gamma, beta, mean, rstd, rows, cols, eps);
    else
      hipLaunchKernelGGL((layer_norm_fwd_kernel<false, false>), dim3(grid),
                         dim3(kBlock), 0, stream, out, x, res, sum_out,
                         gamma, beta, mean, rstd, rows, cols, eps);
  }
}

int64_t epl_layer_norm_bwd_parts(int64_t rows) { return ln_bwd_parts(rows); }

// dadd / dy2 / colsum (with its cs_part plane) are optional and only valid
// on the bf16 fast path (cols % 8 == 0, cols <= 2048); the caller checks.
// The partial planes hold epl_layer_norm_bwd_parts(rows) rows of cols
// floats each.  mode_* (kRedAccF32 / kRedStoreF32 / kRedStoreBF16) say how
// dgamma, dbeta and colsum are left; the generic path below accumulates
// into pre-zeroed fp32 and knows no other.
void epl_layer_norm_bwd_fused(void* dx, void* dgamma, void* dbeta,
                              void* colsum, int mode_g, int mode_b,
                              int mode_c, const void* dy, const void* dy2,
                              const void* x, const void* gamma,
                              const void* dadd, const float* mean,
                              const float* rstd, float* dg_part,
                              float* db_part, float* cs_part, int64_t rows,
                              int64_t cols, bool bf16, hipStream_t stream) {
  if (bf16 && cols % 8 == 0 && cols <= 2048 && dg_part != nullptr) {
    const bool has_cs = colsum != nullptr && cs_part != nullptr;
    LnBwdArgs a;
    a.dx = dx;
    a.outs.p[0] = {dgamma, dg_part, mode_g};
    a.outs.p[1] = {dbeta, db_part, mode_b};
    a.outs.p[2] = {has_cs ? colsum : nullptr, has_cs ? cs_part : nullptr,
                   mode_c};
    a.dy = dy; a.dy2 = dy2; a.x = x; a.gamma = gamma; a.dadd = dadd;
    a.mean = mean; a.rstd = rstd;
    a.rows = rows; a.cols = cols; a.stream = stream;
    if (dadd != nullptr) {
      if (has_cs) ln_bwd_fast_dy2<true, true>(a);
      else ln_bwd_fast_dy2<true, false>(a);
    } else {
      if (has_cs) ln_bwd_fast_dy2<false, true>(a);
      else ln_bwd_fast_dy2<false, false>(a);
    }
    return;
  }
  int grid = (int)(rows < 1024 ? rows : 1024);
  const size_t lds_bytes = (size_t)cols * 2 * sizeof(float);
  float* dg = reinterpret_cast<float*>(dgamma);
  float* db = reinterpret_cast<float*>(dbeta);
  if (bf16)
    hipLaunchKernelGGL((layer_norm_bwd_kernel<true>), dim3(grid),
                       dim3(kBlock), lds_bytes, stream, dx, dg, db,
                       dy, x, gamma, mean, rstd, rows, cols);
  else
    hipLaunchKernelGGL((layer_norm_bwd_kernel<false>), dim3(grid),
                       dim3(kBlock), lds_bytes, stream, dx, dg, db,
                       dy, x, gamma, mean, rstd, rows, cols);
}

void epl_layer_norm_bwd(void* dx, float* dgamma, float* dbeta, const void* dy,
                        const void* x, const void* gamma, const float* mean,
                        const float* rstd, float* dg_part, float* db_part,
                        int64_t rows, int64_t cols, bool bf16,
                        hipStream_t stream) {
  epl_layer_norm_bwd_fused(dx, dgamma, dbeta, nullptr, kRedAccF32,
                           kRedAccF32, kRedAccF32, dy, nullptr, x, gamma,
                           nullptr, mean, rstd, dg_part, db_part, nullptr,
                           rows, cols, bf16, stream);
}

void epl_bias_gelu_fwd(void* out, const void* x, const void* bias,
                       int64_t rows, int64_t cols, bool bf16,
                       hipStream_t stream) {
  int grid = grid_for((rows * cols + 7) / 8);
  if (bf16) {
    // the kernel tiles whole rows: it needs at least one row of threads
    const int min_grid = (int)((cols / 8 + kBlock - 1) / kBlock);
    if (grid < min_grid) grid = min_grid;
    hipLaunchKernelGGL(bias_gelu_fwd_kernel<true>, dim3(grid), dim3(kBlock), 0,
                       stream, out, x, bias, rows, cols);
  } else
    hipLaunchKernelGGL(bias_gelu_fwd_kernel<false>, dim3(grid), dim3(kBlock),
                       0, stream, out, x, bias, rows, cols);
}

// partial rows per 512-column segment of the bf16 fast backward
int64_t epl_bias_gelu_bwd_parts(int64_t rows) {
  int64_t per_seg = rows < 1024 ? (rows > 0 ? rows : 1) : 1024;
  return (per_seg + 3) / 4 * 4;   // whole blocks for every segment count
}

// db_part: [epl_bias_gelu_bwd_parts(rows), cols] floats, fast path only
// (bf16, cols % 512 == 0).  mode: how dbias is left (kRed*); the generic
// path accumulates into pre-zeroed fp32 and knows no other.
void epl_bias_gelu_bwd(void* dx, void* dbias, int mode, const void* dy,
                       const void* x, const void* bias, float* db_part,
                       int64_t rows, int64_t cols, bool bf16,
                       hipStream_t stream) {
  if (bf16 && cols % 512 == 0 && db_part != nullptr) {
    const int64_t segs = cols / 512;
    const int64_t per_seg = epl_bias_gelu_bwd_parts(rows);
    const int grid = (int)(segs * per_seg / 4);
    hipLaunchKernelGGL(bias_gelu_bwd_bf16_kernel, dim3(grid), dim3(256), 0,
                       stream, dx, db_part, dy, x, bias, rows, cols);
    RedPlanes outs;
    outs.p[0] = {dbias, db_part, mode};
    outs.p[1] = outs.p[2] = {nullptr, nullptr, mode};
    hipLaunchKernelGGL(partial_rows_reduce_kernel,
                       dim3((unsigned)((cols + kRedCols - 1) / kRedCols), 1),
                       dim3(kRedCols * kRedSlices), 0,
                       stream, outs, per_seg, cols);
    return;
  }
  int grid = (int)(rows < 1024 ? rows : 1024);
  const size_t lds_bytes = (size_t)cols * sizeof(float);
  float* db = reinterpret_cast<float*>(dbias);
  if (bf16)
    hipLaunchKernelGGL(bias_gelu_bwd_kernel<true>, dim3(grid), dim3(kBlock),
                       lds_bytes, stream, dx, db, dy, x, bias, rows, cols);
  else
    hipLaunchKernelGGL(bias_gelu_bwd_kernel<false>, dim3(grid), dim3(kBlock),
                       lds_bytes, stream, dx, db, dy, x, bias, rows, cols);
}

void epl_ce_rowstats(const void* logits, const int64_t* targets,
                     float* row_max, float* row_sumexp, float* target_logit,
                     int64_t rows, int64_t cols, int64_t vocab_begin,
                     int64_t ignore_index, bool skip_ignored, bool bf16,
                     hipStream_t stream) {
  const int grid = (int)(rows < kMaxGrid ? rows : kMaxGrid);
  if (bf16)
    hipLaunchKernelGGL(ce_rowstats_kernel<true>, dim3(grid), dim3(kBlock), 0,
                       stream, logits, targets, row_max, row_sumexp,
                       target_logit, rows, cols, vocab_begin, ignore_index,
                       skip_ignored);
  else
    hipLaunchKernelGGL(ce_rowstats_kernel<false>, dim3(grid), dim3(kBlock), 0,
                       stream, logits, targets, row_max, row_sumexp,
                       target_logit, rows, cols, vocab_begin, ignore_index,
                       skip_ignored);
}

void epl_ce_backward(void* dlogits, const void* logits, const int64_t* targets,
                     const float* gmax, const float* gsumexp,
                     const float* dloss, int64_t rows, int64_t cols,
                     int64_t vocab_begin, int64_t ignore_index, float scale,
                     bool bf16, hipStream_t stream) {
  const int grid = (int)(rows < kMaxGrid ? rows : kMaxGrid);
  if (bf16)
    hipLaunchKernelGGL(ce_backward_kernel<true>, dim3(grid), dim3(kBlock), 0,
                       stream, dlogits, logits, targets, gmax, gsumexp, dloss,
                       rows, cols, vocab_begin, ignore_index, scale);
  else
    hipLaunchKernelGGL(ce_backward_kernel<false>, dim3(grid), dim3(kBlock), 0,
                       stream, dlogits, logits, targets, gmax, gsumexp, dloss,
                       rows, cols, vocab_begin, ignore_index, scale);
}

void epl_scale(void* p, int64_t n, float s, bool bf16, hipStream_t stream) {
  const int grid = grid_for((n + 7) / 8);
  if (bf16)
    hipLaunchKernelGGL(scale_bf16_kernel, dim3(grid), dim3(kBlock), 0, stream,
                       reinterpret_cast<unsigned short*>(p), n, s);
  else
    hipLaunchKernelGGL(scale_f32_kernel, dim3(grid), dim3(kBlock), 0, stream,
                       reinterpret_cast<float*>(p), n, s);
}

void epl_f32_to_bf16(unsigned short* dst, const float* src, int64_t n,
                     hipStream_t stream) {
  const int grid = grid_for((n + 7) / 8);
  hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(grid), dim3(kBlock), 0, stream,
                     dst, src, n);
}

void epl_bf16_to_f32(float* dst, const unsigned short* src, int64_t n,
                     hipStream_t stream) {
  const int grid = grid_for((n + 7) / 8);
  hipLaunchKernelGGL(bf16_to_f32_kernel, dim3(grid), dim3(kBlock), 0, stream,
                     dst, src, n);
}

void epl_sqnorm(const void* p, int64_t n, float* out, bool bf16,
                hipStream_t stream) {
  const int grid = grid_for(n) < 1024 ? grid_for(n) : 1024;
  if (bf16)
    hipLaunchKernelGGL(sqnorm_kernel<true>, dim3(grid), dim3(kBlock), 0,
                       stream, p, n, out);
  else
    hipLaunchKernelGGL(sqnorm_kernel<false>, dim3(grid), dim3(kBlock), 0,
                       stream, p, n, out);
}


void epl_colsum(void* db, const void* dy, float* partial, int64_t rows,
                int64_t cols, int64_t stripes, bool bf16,
                hipStream_t stream) {
  // size the block to the column count so narrow matrices (cols/8 < 256
  // lanes) don't launch half-idle blocks
  int64_t thr = cols / 8;
  thr = thr < 64 ? 64 : (thr > 256 ? 256 : thr);
  thr = (thr + 63) / 64 * 64;
  dim3 grid((unsigned)((cols / 8 + thr - 1) / thr), (unsigned)stripes);
  if (bf16)
    hipLaunchKernelGGL((colsum_partial_kernel<true>), grid, dim3((unsigned)thr),
                       0, stream, dy, partial, rows, cols, stripes);
  else
    hipLaunchKernelGGL((colsum_partial_kernel<false>), grid,
                       dim3((unsigned)thr), 0, stream, dy, partial, rows,
                       cols, stripes);
  dim3 rgrid((unsigned)((cols + 255) / 256));
  if (bf16)
    hipLaunchKernelGGL((colsum_reduce_kernel<true>), rgrid, dim3(256), 0,
                       stream, db, partial, stripes, cols);
  else
    hipLaunchKernelGGL((colsum_reduce_kernel<false>), rgrid, dim3(256), 0,
                       stream, db, partial, stripes, cols);
}

}  // extern "C"
