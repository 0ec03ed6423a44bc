// Fused MoE router (gfx950): softmax, top-1/top-2 selection, combine
// weights, per-expert counts, load-balance loss and z loss in one forward
// pass over the gate logits, and one backward pass that writes dlogits.
// The semantics are fixed in easyparallellibrary_amd/ops/moe.py.
//
// Layout: a token is owned by a group of G lanes (G a power of two, 1 up
// to a whole 64-lane wave), lane l of the group holding the V consecutive
// experts [l*V, l*V+V) in registers; experts >= E are padded with -inf.
// G*V >= E with V = 8 up to E = 128 and V = 4 (G = 64) above, so at E = 8
// bf16 a lane loads its token's whole row as one 16-byte vector and a
// wave covers 64 consecutive rows with one 1 KiB load.  When E % V != 0
// the row is read element by element (rows are not 16-byte aligned then).
// Sum and top-2 merge cross the group with __shfl_xor; the token loop is
// grid-stride, wave-uniform, and has no LDS and no barrier.
//
// Column reductions (sum_t p_te, the counts, sum_t lse_t^2) follow the
// LayerNorm-backward rule: registers across the wave's tokens, a fixed
// xor tree across the wave's groups, one PARTIAL ROW per wave in a
// workspace, and a small second kernel that folds the rows in a fixed
// order.  No float atomics: results are bitwise reproducible.

#include <hip/hip_runtime.h>
#include <cstdint>

namespace {

constexpr int kThreads = 256;
constexpr int kWavesPerBlock = kThreads / 64;
constexpr int kMaxBlocks = 256;   // one block per CU; the rest grid-strides
constexpr int kBig = 0x7fffffff;

__device__ __forceinline__ float rbf2f(unsigned short u) {
  union { unsigned int i; float f; } v;
  v.i = ((unsigned int)u) << 16;
  return v.f;
}

__device__ __forceinline__ unsigned short rf2bf(float f) {
  union { float f; unsigned int i; } v;
  v.f = f;
  if ((v.i & 0x7fffffffu) > 0x7f800000u)      // NaN stays NaN
    return (unsigned short)((v.i >> 16) | 0x40u);
  unsigned int lsb = (v.i >> 16) & 1u;
  return (unsigned short)((v.i + 0x7fffu + lsb) >> 16);
}

template <int V> struct BfVec;
template <> struct BfVec<8> {
  using type = __attribute__((ext_vector_type(8))) unsigned short;
};
template <> struct BfVec<4> {
  using type = __attribute__((ext_vector_type(4))) unsigned short;
};
using f32x4 = __attribute__((ext_vector_type(4))) float;

// z[v] = logits[row][e0 + v] as float, -inf at experts >= E (and for a
// token past the end, whose results are never stored)
template <int V>
__device__ __forceinline__ void load_row(float (&z)[V], const float* row,
                                         int e0, int E, bool vec,
                                         bool live) {
#pragma unroll
  for (int v = 0; v < V; ++v) z[v] = -INFINITY;
  if (!live || e0 >= E) return;
  if (vec) {
#pragma unroll
    for (int q = 0; q < V / 4; ++q) {
      f32x4 x = *reinterpret_cast<const f32x4*>(row + e0 + 4 * q);
#pragma unroll
      for (int v = 0; v < 4; ++v) z[4 * q + v] = x[v];
    }
  } else {
#pragma unroll
    for (int v = 0; v < V; ++v)
      if (e0 + v < E) z[v] = row[e0 + v];
  }
}

template <int V>
__device__ __forceinline__ void load_row(float (&z)[V],
                                         const unsigned short* row, int e0,
                                         int E, bool vec, bool live) {
#pragma unroll
  for (int v = 0; v < V; ++v) z[v] = -INFINITY;
  if (!live || e0 >= E) return;
  if (vec) {
    typename BfVec<V>::type x =
        *reinterpret_cast<const typename BfVec<V>::type*>(row + e0);
#pragma unroll
    for (int v = 0; v < V; ++v) z[v] = rbf2f(x[v]);
  } else {
#pragma unroll
    for (int v = 0; v < V; ++v)
      if (e0 + v < E) z[v] = rbf2f(row[e0 + v]);
  }
}

template <int V>
__device__ __forceinline__ void store_row(const float (&d)[V], float* row,
                                          int e0, int E, bool vec) {
  if (e0 >= E) return;
  if (vec) {
#pragma unroll
    for (int q = 0; q < V / 4; ++q) {
      f32x4 x;
#pragma unroll
      for (int v = 0; v < 4; ++v) x[v] = d[4 * q + v];
      *reinterpret_cast<f32x4*>(row + e0 + 4 * q) = x;
    }
  } else {
#pragma unroll
    for (int v = 0; v < V; ++v)
      if (e0 + v < E) row[e0 + v] = d[v];
  }
}

template <int V>
__device__ __forceinline__ void store_row(const float (&d)[V],
                                          unsigned short* row, int e0,
                                          int E, bool vec) {
  if (e0 >= E) return;
  if (vec) {
    typename BfVec<V>::type x;
#pragma unroll
    for (int v = 0; v < V; ++v) x[v] = rf2bf(d[v]);
    *reinterpret_cast<typename BfVec<V>::type*>(row + e0) = x;
  } else {
#pragma unroll
    for (int v = 0; v < V; ++v)
      if (e0 + v < E) row[e0 + v] = rf2bf(d[v]);
  }
}

// (value, index) a ranks before b: larger value, ties to the lower index
__device__ __forceinline__ bool before(float av, int ai, float bv, int bi) {
  return av > bv || (av == bv && ai < bi);
}

template <int G>
__device__ __forceinline__ float group_sum(float x) {
#pragma unroll
  for (int off = 1; off < G; off <<= 1) x += __shfl_xor(x, off, 64);
  return x;
}

// Forward.  Per token: topi int64 [N, K], topw fp32 [N, K], lse fp32 [N].
// Per wave: partial rows p_part [waves, E], c_part [waves, E] (int32),
// z_part [waves].
template <typename T, int G, int V, int K>
__global__ void __launch_bounds__(kThreads) moe_router_fwd_kernel(
    const T* __restrict__ logits, int64_t* __restrict__ topi,
    float* __restrict__ topw, float* __restrict__ lse_out,
    float* __restrict__ p_part, int* __restrict__ c_part,
    float* __restrict__ z_part, int64_t N, int E, bool vec) {
  constexpr int TPW = 64 / G;                    // tokens per wave and pass
  const int lane = threadIdx.x & 63;
  const int gl = lane & (G - 1);                 // lane within the group
  const int e0 = gl * V;
  const int64_t wave = ((int64_t)blockIdx.x * kThreads + threadIdx.x) >> 6;
  const int64_t waves = (int64_t)gridDim.x * kWavesPerBlock;
  float pacc[V];
  int cacc[V];
#pragma unroll
  for (int v = 0; v < V; ++v) { pacc[v] = 0.f; cacc[v] = 0; }
  float zacc = 0.f;

  for (int64_t base = wave * TPW; base < N; base += waves * TPW) {
    const int64_t t = base + lane / G;
    const bool live = t < N;
    float z[V];
    load_row<V>(z, logits + (live ? t : 0) * E, e0, E, vec, live);
    // the lane's own two best, scanning upwards so ties keep the lower index
    float v1 = -INFINITY, v2 = -INFINITY;
    int i1 = kBig, i2 = kBig;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int e = e0 + v < E ? e0 + v : kBig;
      if (before(z[v], e, v1, i1)) {
        v2 = v1; i2 = i1; v1 = z[v]; i1 = e;
      } else if (before(z[v], e, v2, i2)) {
        v2 = z[v]; i2 = e;
      }
    }
    // merge across the group: (value desc, index asc) is a total order
    // on distinct indices, so both partners compute the same pair
#pragma unroll
    for (int off = 1; off < G; off <<= 1) {
      const float ov1 = __shfl_xor(v1, off, 64);
      const float ov2 = __shfl_xor(v2, off, 64);
      const int oi1 = __shfl_xor(i1, off, 64);
      const int oi2 = __shfl_xor(i2, off, 64);
      if (before(ov1, oi1, v1, i1)) {
        // theirs first; second is the better of their second and my first
        if (before(ov2, oi2, v1, i1)) { v2 = ov2; i2 = oi2; }
        else { v2 = v1; i2 = i1; }
        v1 = ov1; i1 = oi1;
      } else if (before(ov1, oi1, v2, i2)) {
        v2 = ov1; i2 = oi1;
      }
    }
    const float m = live ? v1 : 0.f;
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) s += expf(z[v] - m);
    s = group_sum<G>(s);
    const float lse = live ? m + logf(s) : 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      pacc[v] += expf(z[v] - lse);               // 0 at padding and dead rows
      if (live)
        cacc[v] += (e0 + v == i1) + (K == 2 && e0 + v == i2);
    }
    if (live && gl == 0) {
      zacc += lse * lse;
      lse_out[t] = lse;
      if (K == 1) {
        topi[t] = i1;
        topw[t] = 1.f;
      } else {
        const float p1 = expf(v1 - lse), p2 = expf(v2 - lse);
        const float sel = p1 + p2;
        topi[2 * t] = i1;
        topi[2 * t + 1] = i2;
        topw[2 * t] = p1 / sel;
        topw[2 * t + 1] = p2 / sel;
      }
    }
  }
  // fold the wave's groups in a fixed xor tree, then one partial row
#pragma unroll
  for (int off = G; off < 64; off <<= 1) {
#pragma unroll
    for (int v = 0; v < V; ++v) {
      pacc[v] += __shfl_xor(pacc[v], off, 64);
      cacc[v] += __shfl_xor(cacc[v], off, 64);
    }
    zacc += __shfl_xor(zacc, off, 64);
  }
  if (lane < G) {
#pragma unroll
    for (int v = 0; v < V; ++v)
      if (e0 + v < E) {
        p_part[wave * E + e0 + v] = pacc[v];
        c_part[wave * E + e0 + v] = cacc[v];
      }
  }
  if (lane == 0) z_part[wave] = zacc;
}

// Folds the partial rows in a fixed order: thread (slice, column) sums
// rows slice, slice + S, ... of its column, the slices meet in an LDS
// tree.  Then L_bal = E sum_e (c_e / (N K)) (psum_e / N) and
// L_z = sum lse^2 / N, each by the same fixed tree.  One block, EP = the
// power of two >= E.
__global__ void __launch_bounds__(kThreads) moe_router_reduce_kernel(
    const float* __restrict__ p_part, const int* __restrict__ c_part,
    const float* __restrict__ z_part, int64_t* __restrict__ counts,
    float* __restrict__ psum, float* __restrict__ losses, int waves,
    int64_t N, int E, int EP, int K) {
  __shared__ float sp[kThreads];
  __shared__ int sc[kThreads];
  const int tid = threadIdx.x;
  const int col = tid & (EP - 1);
  const int slice = tid / EP;
  const int slices = kThreads / EP;
  float p = 0.f;
  int c = 0;
  if (col < E)
    for (int r = slice; r < waves; r += slices) {
      p += p_part[(int64_t)r * E + col];
      c += c_part[(int64_t)r * E + col];
    }
  sp[tid] = p;
  sc[tid] = c;
  __syncthreads();
  for (int half = kThreads / 2; half >= EP; half >>= 1) {
    if (tid < half) {
      sp[tid] += sp[tid + half];
      sc[tid] += sc[tid + half];
    }
    __syncthreads();
  }
  // sp[0..EP) / sc[0..EP) now hold the column totals
  float term = 0.f;
  if (tid < E) {
    const float ps = sp[tid];
    const int cnt = sc[tid];
    psum[tid] = ps;
    counts[tid] = cnt;
    const float f = (float)cnt / ((float)N * (float)K);
    term = f * (ps / (float)N);
  }
  float zz = 0.f;
  for (int r = tid; r < waves; r += kThreads) zz += z_part[r];
  __syncthreads();
  sp[tid] = term;
  __syncthreads();
  for (int half = kThreads / 2; half >= 1; half >>= 1) {
    if (tid < half) sp[tid] += sp[tid + half];
    __syncthreads();
  }
  const float bal = (float)E * sp[0];
  __syncthreads();
  sp[tid] = zz;
  __syncthreads();
  for (int half = kThreads / 2; half >= 1; half >>= 1) {
    if (tid < half) sp[tid] += sp[tid + half];
    __syncthreads();
  }
  if (tid == 0) {
    losses[0] = bal;
    losses[1] = sp[0] / (float)N;
  }
}

// Backward: p from the saved lse, then
//   a_e  = g_bal E f_e / N  (+ (dw_j - sum_l dw_l w_l) / S at selected e)
//   dz_e = p_e (a_e - sum_e' p_e' a_e') + g_z (2 lse / N) p_e
// rounded once to T.  Every element of dlogits is written.
template <typename T, int G, int V, int K>
__global__ void __launch_bounds__(kThreads) moe_router_bwd_kernel(
    T* __restrict__ dlogits, const T* __restrict__ logits,
    const float* __restrict__ lse_in, const int64_t* __restrict__ topi,
    const float* __restrict__ dw, const int64_t* __restrict__ counts,
    const float* __restrict__ g_bal, const float* __restrict__ g_z,
    int64_t N, int E, bool vec) {
  constexpr int TPW = 64 / G;
  const int lane = threadIdx.x & 63;
  const int gl = lane & (G - 1);
  const int e0 = gl * V;
  const int64_t wave = ((int64_t)blockIdx.x * kThreads + threadIdx.x) >> 6;
  const int64_t waves = (int64_t)gridDim.x * kWavesPerBlock;
  const float fn = (float)N;
  const float gb = g_bal[0];
  const float gz2 = g_z[0] * (2.f / fn);
  float abal[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const float f = e0 + v < E
        ? (float)counts[e0 + v] / (fn * (float)K) : 0.f;
    abal[v] = gb * (float)E * f / fn;
  }
  for (int64_t base = wave * TPW; base < N; base += waves * TPW) {
    const int64_t t = base + lane / G;
    const bool live = t < N;
    const int64_t tt = live ? t : 0;
    float z[V], p[V], a[V];
    load_row<V>(z, logits + tt * E, e0, E, vec, live);
    const float lse = lse_in[tt];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      p[v] = expf(z[v] - lse);
      a[v] = abal[v];
    }
    if (K == 2) {
      const int i1 = (int)topi[2 * tt], i2 = (int)topi[2 * tt + 1];
      const float d1 = dw[2 * tt], d2 = dw[2 * tt + 1];
      float p1 = 0.f, p2 = 0.f;
#pragma unroll
      for (int v = 0; v < V; ++v) {
        p1 += e0 + v == i1 ? p[v] : 0.f;
        p2 += e0 + v == i2 ? p[v] : 0.f;
      }
      p1 = group_sum<G>(p1);       // one non-zero term each: exact
      p2 = group_sum<G>(p2);
      const float sel = p1 + p2;
      const float dot = d1 * (p1 / sel) + d2 * (p2 / sel);
      const float a1 = (d1 - dot) / sel, a2 = (d2 - dot) / sel;
#pragma unroll
      for (int v = 0; v < V; ++v) {
        a[v] += e0 + v == i1 ? a1 : 0.f;
        a[v] += e0 + v == i2 ? a2 : 0.f;
      }
    }
    float pa = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) pa += p[v] * a[v];
    pa = group_sum<G>(pa);
    const float gl2 = gz2 * lse;
    float d[V];
#pragma unroll
    for (int v = 0; v < V; ++v) d[v] = p[v] * (a[v] - pa) + gl2 * p[v];
    if (live) store_row<V>(d, dlogits + t * E, e0, E, vec);
  }
}

int router_blocks(int64_t N, int G) {
  const int64_t per_block = (int64_t)kWavesPerBlock * (64 / G);
  int64_t blocks = (N + per_block - 1) / per_block;
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

// lanes per token and experts per lane for E experts
void router_shape(int E, int* G, int* V) {
  if (E > 128) { *G = 64; *V = 4; return; }
  *V = 8;
  int g = 1;
  while (g * 8 < E) g <<= 1;
  *G = g;
}

template <typename T, int G, int V>
void launch_fwd(const void* logits, int64_t* topi, float* topw, float* lse,
                float* p_part, int* c_part, float* z_part, int64_t N, int E,
                int K, bool vec, int blocks, hipStream_t stream) {
  const T* lg = reinterpret_cast<const T*>(logits);
  if (K == 1)
    hipLaunchKernelGGL((moe_router_fwd_kernel<T, G, V, 1>), dim3(blocks),
                       dim3(kThreads), 0, stream, lg, topi, topw, lse,
                       p_part, c_part, z_part, N, E, vec);
  else
    hipLaunchKernelGGL((moe_router_fwd_kernel<T, G, V, 2>), dim3(blocks),
                       dim3(kThreads), 0, stream, lg, topi, topw, lse,
                       p_part, c_part, z_part, N, E, vec);
}

template <typename T, int G, int V>
void launch_bwd(void* dlogits, const void* logits, const float* lse,
                const int64_t* topi, const float* dw, const int64_t* counts,
                const float* g_bal, const float* g_z, int64_t N, int E,
                int K, bool vec, int blocks, hipStream_t stream) {
  T* dl = reinterpret_cast<T*>(dlogits);
  const T* lg = reinterpret_cast<const T*>(logits);
  if (K == 1)
    hipLaunchKernelGGL((moe_router_bwd_kernel<T, G, V, 1>), dim3(blocks),
                       dim3(kThreads), 0, stream, dl, lg, lse, topi, dw,
                       counts, g_bal, g_z, N, E, vec);
  else
    hipLaunchKernelGGL((moe_router_bwd_kernel<T, G, V, 2>), dim3(blocks),
                       dim3(kThreads), 0, stream, dl, lg, lse, topi, dw,
                       counts, g_bal, g_z, N, E, vec);
}

#define ROUTER_DISPATCH(FN, T, ...)                              \
  switch (G) {                                                   \
    case 1: FN<T, 1, 8>(__VA_ARGS__); break;                     \
    case 2: FN<T, 2, 8>(__VA_ARGS__); break;                     \
    case 4: FN<T, 4, 8>(__VA_ARGS__); break;                     \
    case 8: FN<T, 8, 8>(__VA_ARGS__); break;                     \
    case 16: FN<T, 16, 8>(__VA_ARGS__); break;                   \
    default: FN<T, 64, 4>(__VA_ARGS__); break;                   \
  }

}  // namespace

extern "C" {

// partial rows (= waves) the forward writes for N tokens of E experts
int64_t epl_moe_router_waves(int64_t N, int64_t E) {
  int G, V;
  router_shape((int)E, &G, &V);
  return (int64_t)router_blocks(N, G) * kWavesPerBlock;
}

// p_part: fp32 [waves * E + waves] (the last `waves` hold sum lse^2),
// c_part: int32 [waves * E]
void epl_moe_router_fwd(const void* logits, int64_t* topi, float* topw,
                        float* lse, int64_t* counts, float* psum,
                        float* losses, float* p_part, int* c_part,
                        int64_t N, int64_t E, int64_t K, bool bf16,
                        bool vec, hipStream_t stream) {
  int G, V;
  router_shape((int)E, &G, &V);
  vec = vec && E % V == 0;
  const int blocks = router_blocks(N, G);
  const int waves = blocks * kWavesPerBlock;
  float* z_part = p_part + (int64_t)waves * E;
  if (bf16) {
    ROUTER_DISPATCH(launch_fwd, unsigned short, logits, topi, topw, lse,
                    p_part, c_part, z_part, N, (int)E, (int)K, vec, blocks,
                    stream)
  } else {
    ROUTER_DISPATCH(launch_fwd, float, logits, topi, topw, lse, p_part,
                    c_part, z_part, N, (int)E, (int)K, vec, blocks, stream)
  }
  int EP = 1;
  while (EP < E) EP <<= 1;
  hipLaunchKernelGGL(moe_router_reduce_kernel, dim3(1), dim3(kThreads), 0,
                     stream, p_part, c_part, z_part, counts, psum, losses,
                     waves, N, (int)E, EP, (int)K);
}

void epl_moe_router_bwd(void* dlogits, const void* logits, const float* lse,
                        const int64_t* topi, const float* dw,
                        const int64_t* counts, const float* g_bal,
                        const float* g_z, int64_t N, int64_t E, int64_t K,
                        bool bf16, bool vec, hipStream_t stream) {
  int G, V;
  router_shape((int)E, &G, &V);
  vec = vec && E % V == 0;
  const int blocks = router_blocks(N, G);
  if (bf16) {
    ROUTER_DISPATCH(launch_bwd, unsigned short, dlogits, logits, lse, topi,
                    dw, counts, g_bal, g_z, N, (int)E, (int)K, vec, blocks,
                    stream)
  } else {
    ROUTER_DISPATCH(launch_bwd, float, dlogits, logits, lse, topi, dw,
                    counts, g_bal, g_z, N, (int)E, (int)K, vec, blocks,
                    stream)
  }
}

}  // extern "C"
