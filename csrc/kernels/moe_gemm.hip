// Grouped GEMM of the MoE expert FFN (gfx950, bf16 operands, fp32 MFMA
// accumulation, one v_cvt_pk_bf16_f32 rounding per stored element).
//
// E experts of M rows each (M is the row pitch), contiguous tensors, and a
// nullable device vector rows[E]: expert e holds m_e = clamp(rows[e], 0, M)
// live leading rows (m_e = M without rows).  Three forms:
//
//   nn  C[e] = A[e] B[e]        A [E,M,K]  B [E,K,N]  C [E,M,N]  forwards
//   nt  C[e] = A[e] B[e]^T      A [E,M,N]  B [E,K,N]  C [E,M,K]  dgrads
//   tn  C[e] = A[e][:m_e]^T B[e][:m_e]
//                               A [E,M,K]  B [E,M,N]  C [E,K,N]  wgrads
//
// One kernel body serves all three.  Write the product as
// C[p][q] = sum_r X[p][r] Y[q][r]; a form says only which index of each
// operand is contiguous in memory (XTR / YTR: the contraction index r is
// NOT the contiguous one) and where the row count applies:
//
//   nn  X = A (p = m, r = k)        Y = B (r = k, q = n, YTR)   rows on p
//   nt  X = A (p = m, r = n)        Y = B (q = k, r = n)        rows on p
//   tn  X = A (r = m, p = k, XTR)   Y = B (r = m, q = n, YTR)   rows on r
//
// Work split.  A block of 256 threads owns a 128 x 128 tile of one
// expert's C for the whole contraction (no split-K, no atomics: every
// element is written once, the sum has one fixed order, two runs agree
// bitwise).  The four waves own its four 64 x 64 quadrants, each as 2 x 2
// MFMA tiles of 32 x 32 (64 accumulator VGPRs).  The MFMA computes the
// transposed tile, D[q][p] with Y as its first operand: a lane then holds
// one C row and 4 consecutive columns per register group, so the store is
// packed 8-byte pieces of row-major C with no shuffle.
//
// Data movement.  The contraction advances 64 at a time.  Each step's
// 128 x 64 tiles of X and Y are staged exactly as they lie in memory
// (16-byte global loads along the contiguous index, no transpose in global
// memory, no operand copy) into the two images of moe_gemm_lds.h; an
// operand whose contraction index is not contiguous is read back with the
// transposed LDS read.  Staging is the register-prefetch / alternate-buffer
// / one-barrier-per-step form of the attention forward and dV kernels:
//
//   barrier; issue the global loads of step s + 1 into registers;
//   16 MFMA-pairs on buffer s & 1; store the registers to buffer (s+1) & 1
//
// The barrier at the top of step s + 1 orders those stores before their
// reads, and the reads of buffer (s + 1) & 1 in step s - 1 before the
// stores (every wave passed the barrier of step s in between).
// 2 buffers x 2 operands x 16 KiB = 64 KiB of LDS, two blocks per CU.
//
// Masking is confined to where it can apply.  The body is compiled twice:
// for blocks whose tile lies inside the live extent (no per-element test
// anywhere) and for edge blocks (last row tile of an expert, partial last
// column tile: row / column indices clamp to the last live one and the
// loaded values are zeroed, so a dead row is never read and a NaN in one
// cannot reach an MFMA).  The contraction loop is peeled: its bulk has
// unconditional loads; only the last step of tn, which may hold fewer than
// 64 live rows, clamps and zeroes by row.  A wave whose whole quadrant is
// dead or outside C skips its MFMAs (wave-uniform; it still stages).
//
// Dead output.  Rows >= m_e of an nn / nt output are written as +0 (the
// caller allocates with torch.empty), without reading `pre` there.  A
// block whose whole row tile is dead writes its zeros and returns before
// any barrier; so does a tn block of an expert with m_e = 0.
//
// Epilogues, both the exact erf GeLU, in fp32 before the single rounding:
//   nn + act:  C = acc, act = gelu(acc)
//   nt + pre:  C = acc * gelu'(pre)
//
// Block order.  The grid is dim3(row tiles, E * column tiles) and the
// linear block id goes through attn_order::block_of: the row tiles of one
// (expert, column tile) follow each other on ONE XCD, so the Y tile they
// share (a 64-deep slab of the expert's weight in nn / nt) is fetched into
// one L2, and eight different (expert, column tile) slabs are in flight
// across the eight XCDs.  It is an index permutation only (bijection
// proved in attn_block_order.h).

#include <hip/hip_runtime.h>
#include <cstdint>

#include "attn_block_order.h"
#include "moe_gemm_lds.h"

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x2 = __attribute__((ext_vector_type(2))) float;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned int;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
using bf16v2 = __attribute__((ext_vector_type(2))) __bf16;

#define DEVI __device__ __forceinline__

namespace {

constexpr int kTile = 128;    // block tile, rows and columns
constexpr int kStep = 64;     // contraction elements per step
constexpr int EPI_NONE = 0, EPI_ACT = 1, EPI_PRE = 2;

struct GemmArgs {
  const short* x;
  const short* y;
  short* c;
  short* act;          // EPI_ACT: second output, like c
  const short* pre;    // EPI_PRE: input, like c
  const int* rows;     // nullable
  int M;               // row pitch of the row-counted tensors
  int P, Q, R;         // C is [P][Q] per expert, R the full contraction
  int ldx, ldy;        // row pitch of X and Y in memory
  int64_t sx, sy, sc;  // per-expert strides, elements
  unsigned int n_pt, n_qt;
};

DEVI unsigned int cvt_pk_bf16(float a, float b) {
  f32x2 f = {a, b};
  return __builtin_bit_cast(unsigned int,
                            __builtin_convertvector(f, bf16v2));
}

DEVI float bf_lo(unsigned int w) { return __uint_as_float(w << 16); }
DEVI float bf_hi(unsigned int w) { return __uint_as_float(w & 0xffff0000u); }

// exact (erf) GeLU and its derivative
DEVI float gelu_f(float x) {
  return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f));
}
DEVI float dgelu_f(float x) {
  return 0.5f * (1.0f + erff(x * 0.70710678118654752f)) +
         x * 0.39894228040143268f * expf(-0.5f * x * x);
}

// This thread's four 16-byte pieces of one operand's 128 x 64 tile per
// step.  ROW image: piece i is chunk t & 7 of tile row (t >> 3) + 32 i.
// TR image: piece i is chunk t & 15 of contraction row (t >> 4) + 16 i.
// The bound on the non-contraction index (idx < idx_lim) never changes
// over the steps, so it is folded into the pointers once.
template <bool TR>
struct Stager {
  const short* p[4];
  bool ok[4];
  int lds[4];
  int64_t step;

  DEVI void init(const short* base, int ld, int idx0, int idx_lim, int t) {
    if (!TR) {
      const int ch = t & 7;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = (t >> 3) + 32 * i;
        int g = idx0 + row;
        ok[i] = g < idx_lim;
        g = ok[i] ? g : idx_lim - 1;
        p[i] = base + (int64_t)g * ld + 8 * ch;
        lds[i] = moe_img::row_off(row, ch);
      }
      step = kStep;
    } else {
      const int ch = t & 15;
      const bool okc = idx0 + 8 * ch < idx_lim;
      const int col = okc ? idx0 + 8 * ch : idx0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = (t >> 4) + 16 * i;
        ok[i] = okc;
        p[i] = base + (int64_t)row * ld + col;
        lds[i] = moe_img::tr_off(row, ch);
      }
      step = (int64_t)kStep * ld;
    }
  }

  // loads of the step whose contraction offset is r0, then advances.
  // EDGE applies the idx bound; TAIL (TR only) the bound r < r_lim on the
  // contraction rows: the row clamps to r_lim - 1 (> r0 - 1, a live row)
  // and the value is zeroed.
  template <bool EDGE, bool TAIL>
  DEVI void load(u32x4 (&v)[4], int r0, int r_lim, int ld, int t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const short* q = p[i];
      bool o = ok[i];
      if (TR && TAIL) {
        const int over = r0 + (t >> 4) + 16 * i - (r_lim - 1);
        if (over > 0) q -= (int64_t)over * ld;
        o = o && over <= 0;
      }
      u32x4 w = *reinterpret_cast<const u32x4*>(q);
      if (EDGE || (TR && TAIL)) {
        const u32x4 z = {0u, 0u, 0u, 0u};
        w = o ? w : z;
      }
      v[i] = w;
      p[i] += step;
    }
  }

  DEVI void store(short* img, const u32x4 (&v)[4]) const {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<u32x4*>(img + lds[i]) = v[i];
  }
};

// one 64-deep step of this wave's 64 x 64 quadrant (wp, wq in {0, 64})
template <bool XTR, bool YTR>
DEVI void mma_step(f32x16 (&acc)[2][2], const short* imgX, const short* imgY,
                   int wp, int wq, int lane) {
#pragma unroll
  for (int c = 0; c < kStep / 16; ++c) {
    bf16x8 xf[2], yf[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      xf[i] = XTR ? moe_img::tr_frag(imgX, wp + 32 * i, c, lane)
                  : moe_img::row_frag(imgX, wp + 32 * i, c, lane);
      yf[i] = YTR ? moe_img::tr_frag(imgY, wq + 32 * i, c, lane)
                  : moe_img::row_frag(imgY, wq + 32 * i, c, lane);
    }
#pragma unroll
    for (int ip = 0; ip < 2; ++ip)
#pragma unroll
      for (int iq = 0; iq < 2; ++iq)
        acc[ip][iq] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            yf[iq], xf[ip], acc[ip][iq], 0, 0, 0);
  }
}

// +0 into rows [p0, p_end) x columns [q0, q_end) of c (and act): 16-byte
// stores, q0 and q_end multiples of 64
template <int EPI>
DEVI void zero_tile(const GemmArgs& a, int64_t cbase, int p0, int p_end,
                    int q0, int q_end, int t) {
  const u32x4 z = {0u, 0u, 0u, 0u};
  const int col = q0 + 8 * (t & 15);
  if (col >= q_end) return;
  for (int row = p0 + (t >> 4); row < p_end; row += 16) {
    const int64_t off = cbase + (int64_t)row * a.Q + col;
    *reinterpret_cast<u32x4*>(a.c + off) = z;
    if (EPI == EPI_ACT) *reinterpret_cast<u32x4*>(a.act + off) = z;
  }
}

template <bool XTR, bool YTR, int EPI, bool EDGE>
DEVI void gemm_body(const GemmArgs& a, short* lds, int e, int p0, int q0,
                    int m_e) {
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wp = 64 * (w & 1), wq = 64 * (w >> 1);
  // rows on p (nn, nt): live output rows m_e, full contraction;
  // rows on r (tn): every output row live, contraction over m_e rows
  const int p_live = XTR ? a.P : m_e;
  const int r_lim = XTR ? m_e : a.R;
  const int steps = (r_lim + kStep - 1) / kStep;

  Stager<XTR> sx;
  Stager<YTR> sy;
  sx.init(a.x + e * a.sx, a.ldx, p0, p_live, t);
  sy.init(a.y + e * a.sy, a.ldy, q0, a.Q, t);

  short* imgX[2] = {lds, lds + 2 * moe_img::kTileShorts};
  short* imgY[2] = {lds + moe_img::kTileShorts,
                    lds + 3 * moe_img::kTileShorts};

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
  const bool wave_live = p0 + wp < p_live && q0 + wq < a.Q;

  u32x4 vx[4], vy[4];
  if (steps == 1) {
    sx.template load<EDGE, true>(vx, 0, r_lim, a.ldx, t);
    sy.template load<EDGE, true>(vy, 0, r_lim, a.ldy, t);
  } else {
    sx.template load<EDGE, false>(vx, 0, r_lim, a.ldx, t);
    sy.template load<EDGE, false>(vy, 0, r_lim, a.ldy, t);
  }
  sx.store(imgX[0], vx);
  sy.store(imgY[0], vy);

  int s = 0;
  // bulk: the loads of step s + 1 are full steps
  for (; s + 2 < steps; ++s) {
    __syncthreads();
    sx.template load<EDGE, false>(vx, (s + 1) * kStep, r_lim, a.ldx, t);
    sy.template load<EDGE, false>(vy, (s + 1) * kStep, r_lim, a.ldy, t);
    if (wave_live)
      mma_step<XTR, YTR>(acc, imgX[s & 1], imgY[s & 1], wp, wq, lane);
    sx.store(imgX[(s + 1) & 1], vx);
    sy.store(imgY[(s + 1) & 1], vy);
  }
  // the step that prefetches the last one (tn: the row-masked tail)
  if (s + 1 < steps) {
    __syncthreads();
    sx.template load<EDGE, true>(vx, (s + 1) * kStep, r_lim, a.ldx, t);
    sy.template load<EDGE, true>(vy, (s + 1) * kStep, r_lim, a.ldy, t);
    if (wave_live)
      mma_step<XTR, YTR>(acc, imgX[s & 1], imgY[s & 1], wp, wq, lane);
    sx.store(imgX[(s + 1) & 1], vx);
    sy.store(imgY[(s + 1) & 1], vy);
    ++s;
  }
  __syncthreads();
  if (wave_live)
    mma_step<XTR, YTR>(acc, imgX[s & 1], imgY[s & 1], wp, wq, lane);

  // epilogue: lane holds C row p and, per register group g, the columns
  // q .. q + 3 with q = 8 g + 4 hi
  const int hi = lane >> 5;
  const int64_t cbase = e * a.sc;
#pragma unroll
  for (int ip = 0; ip < 2; ++ip) {
    const int p = p0 + wp + 32 * ip + (lane & 31);
    if (p >= a.P) continue;
    const bool live = p < p_live;
#pragma unroll
    for (int iq = 0; iq < 2; ++iq) {
      const int qt = q0 + wq + 32 * iq;
      if (qt >= a.Q) continue;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int64_t off = cbase + (int64_t)p * a.Q + qt + 8 * g + 4 * hi;
        float v0 = acc[ip][iq][4 * g], v1 = acc[ip][iq][4 * g + 1];
        float v2 = acc[ip][iq][4 * g + 2], v3 = acc[ip][iq][4 * g + 3];
        u32x2 out = {0u, 0u};
        if (live) {
          if (EPI == EPI_PRE) {
            const u32x2 pr = *reinterpret_cast<const u32x2*>(a.pre + off);
            v0 *= dgelu_f(bf_lo(pr[0]));
            v1 *= dgelu_f(bf_hi(pr[0]));
            v2 *= dgelu_f(bf_lo(pr[1]));
            v3 *= dgelu_f(bf_hi(pr[1]));
          }
          out[0] = cvt_pk_bf16(v0, v1);
          out[1] = cvt_pk_bf16(v2, v3);
        }
        *reinterpret_cast<u32x2*>(a.c + off) = out;
        if (EPI == EPI_ACT) {
          u32x2 ao = {0u, 0u};
          if (live) {
            ao[0] = cvt_pk_bf16(gelu_f(v0), gelu_f(v1));
            ao[1] = cvt_pk_bf16(gelu_f(v2), gelu_f(v3));
          }
          *reinterpret_cast<u32x2*>(a.act + off) = ao;
        }
      }
    }
  }
}

template <bool XTR, bool YTR, int EPI>
__global__ __launch_bounds__(256, 2) void moe_gemm_kernel(GemmArgs a) {
  __shared__ __attribute__((aligned(16))) short
      lds[4 * moe_img::kTileShorts];
  const attn_order::Block b = attn_order::block_of(
      blockIdx.x, blockIdx.y, a.n_pt, gridDim.y);
  const int e = (int)(b.bh / a.n_qt);
  const int q0 = (int)(b.bh % a.n_qt) * kTile;
  const int p0 = (int)b.blk * kTile;
  int m_e = a.M;
  if (a.rows != nullptr) {
    const int n = __builtin_amdgcn_readfirstlane(a.rows[e]);
    m_e = n < 0 ? 0 : (n > a.M ? a.M : n);
  }
  const int q_end = q0 + kTile < a.Q ? q0 + kTile : a.Q;
  const int p_end = p0 + kTile < a.P ? p0 + kTile : a.P;
  // nothing live in this block's tile: zeros, before any barrier
  if (XTR ? m_e == 0 : p0 >= m_e) {
    zero_tile<EPI>(a, e * a.sc, p0, p_end, q0, q_end, threadIdx.x);
    return;
  }
  const int p_live = XTR ? a.P : m_e;
  if (p0 + kTile <= p_live && q0 + kTile <= a.Q)
    gemm_body<XTR, YTR, EPI, false>(a, lds, e, p0, q0, m_e);
  else
    gemm_body<XTR, YTR, EPI, true>(a, lds, e, p0, q0, m_e);
}

template <bool XTR, bool YTR, int EPI>
void launch(const GemmArgs& a, int64_t E, hipStream_t stream) {
  hipLaunchKernelGGL((moe_gemm_kernel<XTR, YTR, EPI>),
                     dim3(a.n_pt, (unsigned int)E * a.n_qt), dim3(256), 0,
                     stream, a);
}

}  // namespace

// form 0 = nn, 1 = nt, 2 = tn (shapes in the header comment); aux is act
// (nn, written) or pre (nt, read) or null.  The binding has checked the
// shapes: K % 64 == 0, N % 64 == 0, grid extents below 65536.
extern "C" void epl_moe_gemm(int form, void* c, const void* a, const void* b,
                             const int* rows, void* aux, int64_t E,
                             int64_t M, int64_t K, int64_t N,
                             hipStream_t stream) {
  GemmArgs g;
  g.x = static_cast<const short*>(a);
  g.y = static_cast<const short*>(b);
  g.c = static_cast<short*>(c);
  g.act = static_cast<short*>(aux);
  g.pre = static_cast<const short*>(aux);
  g.rows = rows;
  g.M = (int)M;
  if (form == 0) {
    g.P = (int)M; g.Q = (int)N; g.R = (int)K;
    g.ldx = (int)K; g.ldy = (int)N;
    g.sx = M * K; g.sy = K * N; g.sc = M * N;
  } else if (form == 1) {
    g.P = (int)M; g.Q = (int)K; g.R = (int)N;
    g.ldx = (int)N; g.ldy = (int)N;
    g.sx = M * N; g.sy = K * N; g.sc = M * K;
  } else {
    g.P = (int)K; g.Q = (int)N; g.R = (int)M;
    g.ldx = (int)K; g.ldy = (int)N;
    g.sx = M * K; g.sy = M * N; g.sc = K * N;
  }
  g.n_pt = (unsigned int)((g.P + kTile - 1) / kTile);
  g.n_qt = (unsigned int)((g.Q + kTile - 1) / kTile);
  if (form == 0) {
    if (aux) launch<false, true, EPI_ACT>(g, E, stream);
    else launch<false, true, EPI_NONE>(g, E, stream);
  } else if (form == 1) {
    if (aux) launch<false, false, EPI_PRE>(g, E, stream);
    else launch<false, false, EPI_NONE>(g, E, stream);
  } else {
    launch<true, true, EPI_NONE>(g, E, stream);
  }
}
