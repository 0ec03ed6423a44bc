// Python bindings for the MI355X-native extension: RCCL comm core
// (csrc/comm/rccl_comm.hip) + CDNA4 HIP kernels (csrc/kernels/kernels.hip).

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <cstdint>

#include "kernels/attn_block_order.h"

namespace epl {
void register_comm(py::module& m);
}

extern "C" {
void epl_fused_adamw(float*, unsigned short*, const void*, bool, float*,
                     float*, int64_t, float, float, float, float, float, int,
                     float, hipStream_t);
void epl_lamb_phase1(const float*, const void*, bool, float*, float*, float*,
                     const int*, float*, float*, int64_t, float, float, float,
                     float, int, float, hipStream_t);
void epl_lamb_phase2(float*, unsigned short*, const float*, const int*,
                     const float*, int64_t, float, hipStream_t);
void epl_layer_norm_fwd(void*, const void*, const void*, void*, const void*,
                        const void*, float*, float*, int64_t, int64_t, float,
                        bool, hipStream_t);
int64_t epl_layer_norm_bwd_parts(int64_t);
void epl_layer_norm_bwd(void*, float*, float*, const void*, const void*,
                        const void*, const float*, const float*, float*,
                        float*, int64_t, int64_t, bool, hipStream_t);
void epl_layer_norm_bwd_fused(void*, void*, void*, void*, int, int, int,
                              const void*, const void*, const void*,
                              const void*, const void*, const float*,
                              const float*, float*, float*, float*, int64_t,
                              int64_t, bool, hipStream_t);
void epl_bias_gelu_fwd(void*, const void*, const void*, int64_t, int64_t,
                       bool, hipStream_t);
int64_t epl_bias_gelu_bwd_parts(int64_t);
void epl_bias_gelu_bwd(void*, void*, int, const void*, const void*,
                       const void*, float*, int64_t, int64_t, bool,
                       hipStream_t);
void epl_ce_rowstats(const void*, const int64_t*, float*, float*, float*,
                     int64_t, int64_t, int64_t, int64_t, bool, bool,
                     hipStream_t);
void epl_ce_backward(void*, const void*, const int64_t*, const float*,
                     const float*, const float*, int64_t, int64_t, int64_t,
                     int64_t, float, bool, hipStream_t);
void epl_scale(void*, int64_t, float, bool, hipStream_t);
void epl_f32_to_bf16(unsigned short*, const float*, int64_t, hipStream_t);
void epl_bf16_to_f32(float*, const unsigned short*, int64_t, hipStream_t);
void epl_sqnorm(const void*, int64_t, float*, bool, hipStream_t);
void epl_colsum(void*, const void*, float*, int64_t, int64_t, int64_t,
                bool, hipStream_t);
void run_mfma_probe(const unsigned short*, const unsigned short*, float*,
                    hipStream_t);
void run_tr_read_probe(short*, short*, int, hipStream_t);
void run_block_order_probe(int*, int, int, hipStream_t);
void epl_moe_dispatch_fwd(void*, const void*, const int64_t*,
                          const int64_t*, const int64_t*, int64_t, int64_t,
                          int64_t, hipStream_t);
void epl_moe_dispatch_bwd(void*, const void*, const int64_t*,
                          const int64_t*, const int64_t*, int64_t, int64_t,
                          int64_t, int64_t, hipStream_t);
void epl_moe_combine_fwd(void*, const void*, const float*, const int64_t*,
                         const int64_t*, const int64_t*, int64_t, int64_t,
                         int64_t, int64_t, hipStream_t);
void epl_moe_combine_bwd(void*, float*, const void*, const void*,
                         const float*, const int64_t*, const int64_t*,
                         const int64_t*, int64_t, int64_t, int64_t,
                         hipStream_t);
int64_t epl_moe_router_waves(int64_t, int64_t);
void epl_moe_router_fwd(const void*, int64_t*, float*, float*, int64_t*,
                        float*, float*, float*, int*, int64_t, int64_t,
                        int64_t, bool, bool, hipStream_t);
void epl_moe_router_bwd(void*, const void*, const float*, const int64_t*,
                        const float*, const int64_t*, const float*,
                        const float*, int64_t, int64_t, int64_t, bool, bool,
                        hipStream_t);
void epl_attn_fwd(const void*, const void*, const void*, void*, float*,
                  int64_t, int64_t, float, bool, int64_t, int64_t,
                  const int64_t*,
                  const int64_t*, unsigned int*, int64_t,
                  unsigned long long, int, float, const int*, hipStream_t);
void epl_attn_bwd(const void*, const void*, const void*, const void*,
                  const void*, const float*, float*, void*, void*, void*,
                  int64_t, int64_t, float, bool, int64_t, const int64_t*,
                  const int64_t*, const int64_t*, const int64_t*, int,
                  const unsigned int*, int64_t, float, int64_t,
                  const float*, const int*, hipStream_t);
void epl_rms_norm_fwd(void*, const void*, const void*, void*, const void*,
                      float*, int64_t, int64_t, float, hipStream_t);
int64_t epl_rms_norm_bwd_parts(int64_t, int64_t);
void epl_rms_norm_bwd(void*, float*, const void*, const void*, const void*,
                      const float*, const void*, float*, int64_t, int64_t,
                      hipStream_t);
void epl_rope(void*, const float*, const float*, int64_t, int64_t, int64_t,
              int64_t, int64_t, int64_t, int64_t, int64_t, bool,
              hipStream_t);
void epl_swiglu_fwd(void*, const void*, int64_t, int64_t, hipStream_t);
void epl_swiglu_bwd(void*, const void*, const void*, int64_t, int64_t,
                    hipStream_t);
}

namespace {

hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
}

void check(const at::Tensor& t, at::ScalarType dtype, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a device tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == dtype, name, " has dtype ", t.scalar_type(),
              ", expected ", dtype);
}

// cuda + contiguous, dtype bf16 or fp32 (returned by is_bf16)
void check_arena(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a device tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// the vector loads and stores of the arena kernels start at the base
void check_aligned(const at::Tensor& t, size_t bytes, const char* name) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % bytes == 0, name,
              " must start on a ", bytes, "-byte boundary");
}

bool is_bf16(const at::Tensor& t) {
  TORCH_CHECK(t.scalar_type() == at::kBFloat16 || t.scalar_type() == at::kFloat,
              "expected bf16 or fp32, got ", t.scalar_type());
  return t.scalar_type() == at::kBFloat16;
}

void fused_adamw(at::Tensor master, c10::optional<at::Tensor> param_bf16,
                 at::Tensor grad, at::Tensor m, at::Tensor v, double lr,
                 double beta1, double beta2, double eps, double weight_decay,
                 int64_t step, double inv_scale) {
  check(master, at::kFloat, "master");
  check(m, at::kFloat, "m");
  check(v, at::kFloat, "v");
  check_arena(grad, "grad");
  const bool gbf = is_bf16(grad);
  unsigned short* pb = nullptr;
  if (param_bf16.has_value()) {
    check(*param_bf16, at::kBFloat16, "param_bf16");
    TORCH_CHECK(param_bf16->numel() == master.numel(),
                "arena size mismatch");
    check_aligned(*param_bf16, 16, "param_bf16");
    pb = reinterpret_cast<unsigned short*>(param_bf16->data_ptr());
  }
  const int64_t n = master.numel();
  TORCH_CHECK(grad.numel() == n && m.numel() == n && v.numel() == n,
              "arena size mismatch");
  // eight elements per access: 32 bytes of fp32, 16 of bf16
  check_aligned(master, 32, "master");
  check_aligned(m, 32, "m");
  check_aligned(v, 32, "v");
  check_aligned(grad, gbf ? 16 : 32, "grad");
  epl_fused_adamw(master.data_ptr<float>(), pb, grad.data_ptr(), gbf,
                  m.data_ptr<float>(), v.data_ptr<float>(), n, (float)lr,
                  (float)beta1, (float)beta2, (float)eps, (float)weight_decay,
                  (int)step, (float)inv_scale, cur_stream());
}

void lamb_phase1(at::Tensor master, at::Tensor grad, at::Tensor m,
                 at::Tensor v, at::Tensor update, at::Tensor chunk_of,
                 at::Tensor wnorm_sq, at::Tensor unorm_sq, double beta1,
                 double beta2, double eps, double weight_decay, int64_t step,
                 double inv_scale) {
  check(master, at::kFloat, "master");
  check(update, at::kFloat, "update");
  check(chunk_of, at::kInt, "chunk_of");
  const bool gbf = is_bf16(grad);
  epl_lamb_phase1(master.data_ptr<float>(), grad.data_ptr(), gbf,
                  m.data_ptr<float>(), v.data_ptr<float>(),
                  update.data_ptr<float>(), chunk_of.data_ptr<int>(),
                  wnorm_sq.data_ptr<float>(), unorm_sq.data_ptr<float>(),
                  master.numel(), (float)beta1, (float)beta2, (float)eps,
                  (float)weight_decay, (int)step, (float)inv_scale,
                  cur_stream());
}

void lamb_phase2(at::Tensor master, c10::optional<at::Tensor> param_bf16,
                 at::Tensor update, at::Tensor chunk_of, at::Tensor ratio,
                 double lr) {
  check(master, at::kFloat, "master");
  unsigned short* pb = nullptr;
  if (param_bf16.has_value())
    pb = reinterpret_cast<unsigned short*>(param_bf16->data_ptr());
  epl_lamb_phase2(master.data_ptr<float>(), pb, update.data_ptr<float>(),
                  chunk_of.data_ptr<int>(), ratio.data_ptr<float>(),
                  master.numel(), (float)lr, cur_stream());
}

void layer_norm_fwd(at::Tensor out, at::Tensor x,
                    c10::optional<at::Tensor> res,
                    c10::optional<at::Tensor> sum_out, at::Tensor gamma,
                    at::Tensor beta, at::Tensor mean, at::Tensor rstd,
                    double eps) {
  const bool bf16 = is_bf16(x);
  const int64_t cols = x.size(-1);
  const int64_t rows = x.numel() / cols;
  TORCH_CHECK(!bf16 || cols % 8 == 0, "bf16 LayerNorm needs cols % 8 == 0");
  check(mean, at::kFloat, "mean");
  check(rstd, at::kFloat, "rstd");
  const void* res_p = nullptr;
  void* sum_p = nullptr;
  if (res.has_value()) {
    TORCH_CHECK(sum_out.has_value(),
                "fused residual LayerNorm needs sum_out");
    TORCH_CHECK(res->numel() == x.numel() && sum_out->numel() == x.numel());
    res_p = res->data_ptr();
    sum_p = sum_out->data_ptr();
  }
  epl_layer_norm_fwd(out.data_ptr(), x.data_ptr(), res_p, sum_p,
                     gamma.data_ptr(), beta.data_ptr(),
                     mean.data_ptr<float>(), rstd.data_ptr<float>(), rows,
                     cols, (float)eps, bf16, cur_stream());
}

// how a reducer leaves an output: the values of kernels.hip's kRed* enum
constexpr int kAccF32 = 0;     // += into pre-zeroed fp32 (older bindings)

// 1 = store fp32, 2 = store bf16 (rounded once), by the tensor's dtype
int store_mode(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a device tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  return is_bf16(t) ? 2 : 1;
}

void layer_norm_bwd(at::Tensor dx, at::Tensor dgamma, at::Tensor dbeta,
                    at::Tensor dy, at::Tensor x, at::Tensor gamma,
                    at::Tensor mean, at::Tensor rstd) {
  const bool bf16 = is_bf16(x);
  const int64_t cols = x.size(-1);
  const int64_t rows = x.numel() / cols;
  TORCH_CHECK(!bf16 || cols % 8 == 0, "bf16 LayerNorm needs cols % 8 == 0");
  TORCH_CHECK((size_t)cols * 2 * sizeof(float) <= 128 * 1024,
              "LayerNorm backward supports cols <= 16384");
  check(dgamma, at::kFloat, "dgamma");
  check(dbeta, at::kFloat, "dbeta");
  float* dgp = nullptr;
  float* dbp = nullptr;
  at::Tensor ws;
  const bool fast = bf16 && cols % 8 == 0 && cols <= 2048;
  if (fast) {
    const int64_t nparts = epl_layer_norm_bwd_parts(rows);
    ws = at::empty({2, nparts, cols}, dgamma.options());
    dgp = ws.data_ptr<float>();
    dbp = dgp + nparts * cols;
  }
  epl_layer_norm_bwd(dx.data_ptr(), dgamma.data_ptr<float>(),
                     dbeta.data_ptr<float>(), dy.data_ptr(), x.data_ptr(),
                     gamma.data_ptr(), mean.data_ptr<float>(),
                     rstd.data_ptr<float>(), dgp, dbp, rows, cols, bf16,
                     cur_stream());
}

// The fused LN backward behind layer_norm_bwd_fused (accumulate = true:
// fp32 outputs, zero-initialised by the caller, any shape) and
// layer_norm_bwd_typed (accumulate = false: outputs written in their own
// dtype, bf16 fast path only).
void ln_bwd_fused_impl(at::Tensor& dx, at::Tensor& dgamma, at::Tensor& dbeta,
                       at::Tensor& dy, at::Tensor& x, at::Tensor& gamma,
                       at::Tensor& mean, at::Tensor& rstd,
                       c10::optional<at::Tensor>& dadd,
                       c10::optional<at::Tensor>& colsum_out,
                       c10::optional<at::Tensor>& dy2, bool accumulate,
                       const char* who) {
  const bool bf16 = is_bf16(x);
  const int64_t cols = x.size(-1);
  const int64_t rows = x.numel() / cols;
  TORCH_CHECK(!bf16 || cols % 8 == 0, "bf16 LayerNorm needs cols % 8 == 0");
  TORCH_CHECK((size_t)cols * 2 * sizeof(float) <= 128 * 1024,
              "LayerNorm backward supports cols <= 16384");
  int mode_g = kAccF32, mode_b = kAccF32, mode_c = kAccF32;
  if (accumulate) {
    check(dgamma, at::kFloat, "dgamma");
    check(dbeta, at::kFloat, "dbeta");
  } else {
    mode_g = store_mode(dgamma, "dgamma");
    mode_b = store_mode(dbeta, "dbeta");
  }
  check(dx, x.scalar_type(), "dx");
  check(dy, x.scalar_type(), "dy");
  check(x, x.scalar_type(), "x");
  check(gamma, x.scalar_type(), "gamma");
  check(mean, at::kFloat, "mean");
  check(rstd, at::kFloat, "rstd");
  TORCH_CHECK(dx.numel() == x.numel() && dy.numel() == x.numel());
  TORCH_CHECK(dgamma.numel() == cols && dbeta.numel() == cols);
  TORCH_CHECK(gamma.numel() == cols && mean.numel() == rows &&
              rstd.numel() == rows);
  const bool fast = bf16 && cols % 8 == 0 && cols <= 2048;
  const bool fused =
      dadd.has_value() || colsum_out.has_value() || dy2.has_value();
  TORCH_CHECK(fast || (!fused && accumulate), who,
              ": dadd / colsum_out / dy2 / typed outputs need the bf16 fast "
              "path (cols % 8 == 0, cols <= 2048)");
  const void* dadd_p = nullptr;
  const void* dy2_p = nullptr;
  void* cs_out = nullptr;
  if (dadd.has_value()) {
    check(*dadd, x.scalar_type(), "dadd");
    TORCH_CHECK(dadd->numel() == x.numel(), "dadd shape mismatch");
    dadd_p = dadd->data_ptr();
  }
  if (dy2.has_value()) {
    check(*dy2, x.scalar_type(), "dy2");
    TORCH_CHECK(dy2->numel() == x.numel(), "dy2 shape mismatch");
    dy2_p = dy2->data_ptr();
  }
  if (colsum_out.has_value()) {
    if (accumulate)
      check(*colsum_out, at::kFloat, "colsum_out");
    else
      mode_c = store_mode(*colsum_out, "colsum_out");
    TORCH_CHECK(colsum_out->numel() == cols, "colsum_out shape mismatch");
    cs_out = colsum_out->data_ptr();
  }
  float* dgp = nullptr;
  float* dbp = nullptr;
  float* csp = nullptr;
  at::Tensor ws;
  if (fast) {
    const int64_t nparts = epl_layer_norm_bwd_parts(rows);
    ws = at::empty({cs_out ? 3 : 2, nparts, cols},
                   x.options().dtype(at::kFloat));
    dgp = ws.data_ptr<float>();
    dbp = dgp + nparts * cols;
    if (cs_out) csp = dbp + nparts * cols;
  }
  epl_layer_norm_bwd_fused(dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                           cs_out, mode_g, mode_b, mode_c, dy.data_ptr(),
                           dy2_p, x.data_ptr(), gamma.data_ptr(), dadd_p,
                           mean.data_ptr<float>(), rstd.data_ptr<float>(),
                           dgp, dbp, csp, rows, cols, bf16, cur_stream());
}

// layer_norm_bwd plus two optional in-kernel fusions on the bf16 fast path
// (cols % 8 == 0, cols <= 2048):
//   dadd       [rows, cols] bf16: dx = LNbwd(dy) + dadd, rounded once;
//   colsum_out [cols] fp32, zero-initialised: += column sum of that dx.
// Asking for either on another shape is an error — the caller keeps the
// separate add / sum there.
void layer_norm_bwd_fused(at::Tensor dx, at::Tensor dgamma, at::Tensor dbeta,
                          at::Tensor dy, at::Tensor x, at::Tensor gamma,
                          at::Tensor mean, at::Tensor rstd,
                          c10::optional<at::Tensor> dadd,
                          c10::optional<at::Tensor> colsum_out) {
  c10::optional<at::Tensor> no_dy2;
  ln_bwd_fused_impl(dx, dgamma, dbeta, dy, x, gamma, mean, rstd, dadd,
                    colsum_out, no_dy2, true, "layer_norm_bwd_fused");
}

// The bf16 fast path alone, with
//   dy2        [rows, cols] bf16: a second upstream gradient, dy + dy2 is
//              formed in fp32 inside the kernel;
//   dgamma, dbeta, colsum_out: bf16 or fp32, each WRITTEN in its own dtype
//              (one rounding of the fp32 sum) — no zero fill before, no
//              cast after, and the same bits on every call.
void layer_norm_bwd_typed(at::Tensor dx, at::Tensor dgamma, at::Tensor dbeta,
                          at::Tensor dy, at::Tensor x, at::Tensor gamma,
                          at::Tensor mean, at::Tensor rstd,
                          c10::optional<at::Tensor> dadd,
                          c10::optional<at::Tensor> colsum_out,
                          c10::optional<at::Tensor> dy2) {
  ln_bwd_fused_impl(dx, dgamma, dbeta, dy, x, gamma, mean, rstd, dadd,
                    colsum_out, dy2, false, "layer_norm_bwd_typed");
}

void bias_gelu_fwd(at::Tensor out, at::Tensor x, at::Tensor bias) {
  const bool bf16 = is_bf16(x);
  const int64_t cols = x.size(-1);
  const int64_t rows = x.numel() / cols;
  TORCH_CHECK(!bf16 || cols % 8 == 0, "bf16 bias_gelu needs cols % 8 == 0");
  epl_bias_gelu_fwd(out.data_ptr(), x.data_ptr(), bias.data_ptr(), rows, cols,
                    bf16, cur_stream());
}

void bias_gelu_bwd_impl(at::Tensor& dx, at::Tensor& dbias, at::Tensor& dy,
                        at::Tensor& x, at::Tensor& bias, bool accumulate) {
  const bool bf16 = is_bf16(x);
  const int64_t cols = x.size(-1);
  const int64_t rows = x.numel() / cols;
  TORCH_CHECK(!bf16 || cols % 8 == 0, "bf16 bias_gelu needs cols % 8 == 0");
  TORCH_CHECK((size_t)cols * sizeof(float) <= 128 * 1024,
              "bias_gelu backward supports cols <= 32768");
  const bool fast = bf16 && cols % 512 == 0;
  int mode = kAccF32;
  if (accumulate) {
    check(dbias, at::kFloat, "dbias");
  } else {
    TORCH_CHECK(fast, "bias_gelu_bwd_typed needs the bf16 fast path "
                      "(cols % 512 == 0)");
    mode = store_mode(dbias, "dbias");
  }
  check(dx, x.scalar_type(), "dx");
  check(dy, x.scalar_type(), "dy");
  check(x, x.scalar_type(), "x");
  check(bias, x.scalar_type(), "bias");
  TORCH_CHECK(dx.numel() == x.numel() && dy.numel() == x.numel());
  TORCH_CHECK(dbias.numel() == cols && bias.numel() == cols);
  float* dbp = nullptr;
  at::Tensor ws;
  if (fast) {
    ws = at::empty({epl_bias_gelu_bwd_parts(rows), cols},
                   x.options().dtype(at::kFloat));
    dbp = ws.data_ptr<float>();
  }
  epl_bias_gelu_bwd(dx.data_ptr(), dbias.data_ptr(), mode, dy.data_ptr(),
                    x.data_ptr(), bias.data_ptr(), dbp, rows, cols, bf16,
                    cur_stream());
}

// dbias: fp32, zero-initialised by the caller
void bias_gelu_bwd(at::Tensor dx, at::Tensor dbias, at::Tensor dy,
                   at::Tensor x, at::Tensor bias) {
  bias_gelu_bwd_impl(dx, dbias, dy, x, bias, true);
}

// bf16 fast path alone: dbias (bf16 or fp32) is written in its own dtype,
// no zero fill before and no cast after
void bias_gelu_bwd_typed(at::Tensor dx, at::Tensor dbias, at::Tensor dy,
                         at::Tensor x, at::Tensor bias) {
  bias_gelu_bwd_impl(dx, dbias, dy, x, bias, false);
}

void ce_rowstats(at::Tensor logits, at::Tensor targets, at::Tensor row_max,
                 at::Tensor row_sumexp, at::Tensor target_logit,
                 int64_t vocab_begin, int64_t ignore_index,
                 bool skip_ignored) {
  const bool bf16 = is_bf16(logits);
  const int64_t cols = logits.size(-1);
  const int64_t rows = logits.numel() / cols;
  check(targets, at::kLong, "targets");
  epl_ce_rowstats(logits.data_ptr(), targets.data_ptr<int64_t>(),
                  row_max.data_ptr<float>(), row_sumexp.data_ptr<float>(),
                  target_logit.data_ptr<float>(), rows, cols, vocab_begin,
                  ignore_index, skip_ignored, bf16, cur_stream());
}

void ce_backward(at::Tensor dlogits, at::Tensor logits, at::Tensor targets,
                 at::Tensor gmax, at::Tensor gsumexp, at::Tensor dloss,
                 int64_t vocab_begin, int64_t ignore_index, double scale) {
  const bool bf16 = is_bf16(logits);
  const int64_t cols = logits.size(-1);
  const int64_t rows = logits.numel() / cols;
  epl_ce_backward(dlogits.data_ptr(), logits.data_ptr(),
                  targets.data_ptr<int64_t>(), gmax.data_ptr<float>(),
                  gsumexp.data_ptr<float>(), dloss.data_ptr<float>(), rows,
                  cols, vocab_begin, ignore_index, (float)scale, bf16,
                  cur_stream());
}

void scale_(at::Tensor t, double s) {
  check_arena(t, "t");
  const bool bf16 = is_bf16(t);
  check_aligned(t, 16, "t");   // float4 / bf16x8 accesses
  epl_scale(t.data_ptr(), t.numel(), (float)s, bf16, cur_stream());
}

void f32_to_bf16(at::Tensor dst, at::Tensor src) {
  check(dst, at::kBFloat16, "dst");
  check(src, at::kFloat, "src");
  TORCH_CHECK(dst.numel() == src.numel());
  check_aligned(dst, 16, "dst");   // bf16x8 stores, float4 loads
  check_aligned(src, 16, "src");
  epl_f32_to_bf16(reinterpret_cast<unsigned short*>(dst.data_ptr()),
                  src.data_ptr<float>(), src.numel(), cur_stream());
}

void bf16_to_f32(at::Tensor dst, at::Tensor src) {
  check(dst, at::kFloat, "dst");
  check(src, at::kBFloat16, "src");
  TORCH_CHECK(dst.numel() == src.numel());
  check_aligned(dst, 16, "dst");   // float4 stores, bf16x8 loads
  check_aligned(src, 16, "src");
  epl_bf16_to_f32(dst.data_ptr<float>(),
                  reinterpret_cast<unsigned short*>(src.data_ptr()),
                  src.numel(), cur_stream());
}

static void attn_strides(const at::Tensor& t, int64_t* out3,
                         const char* name) {
  TORCH_CHECK(t.dim() == 4 && (t.size(3) == 64 || t.size(3) == 128), name,
              " must be [B,H,S,64|128]");
  TORCH_CHECK(t.stride(3) == 1, name, " last dim must be contiguous");
  TORCH_CHECK(t.stride(2) % 8 == 0 && t.stride(1) % 8 == 0,
              name, " row strides must be 16-byte aligned");
  out3[0] = t.stride(0);
  out3[1] = t.stride(1);
  out3[2] = t.stride(2);
}

// The attention kernels put one of (batch*heads, 128-row blocks) on
// gridDim.y, which holds at most 65535 blocks: non-causal launches carry
// batch*heads there, causal ones the row blocks (the combined dK+dV kernel
// is non-causal only).  A launch past the limit fails without a trace and
// leaves the outputs unwritten, so refuse it here.
static void attn_check_grid(int64_t bh, int64_t seq, bool causal) {
  const int64_t nqb = (seq + 127) / 128;
  TORCH_CHECK(nqb <= 65535, "attention: seq ", seq, " needs ", nqb,
              " 128-row blocks, more than the 65535 a launch can hold");
  TORCH_CHECK(causal || bh <= 65535, "attention: non-causal batch*heads ",
              bh, " exceeds the 65535 blocks of gridDim.y");
}

// seqlens: optional int32 [B] valid lengths of a right-padded batch.
// Only its layout is checked here; the values are read (and clamped to
// [0, seq]) by the kernels, so there is no host sync and a captured
// graph replays with whatever lengths the tensor then holds.
static const int* attn_seqlens(const c10::optional<at::Tensor>& seqlens,
                               const at::Tensor& q) {
  if (!seqlens.has_value()) return nullptr;
  check(*seqlens, at::kInt, "seqlens");
  TORCH_CHECK(seqlens->numel() == q.size(0), "seqlens must hold ",
              q.size(0), " lengths (one per sample), got ",
              seqlens->numel());
  TORCH_CHECK(seqlens->device() == q.device(),
              "seqlens must be on the device of q");
  return seqlens->data_ptr<int>();
}

// drop_mask: optional int32 [bh*seq*ceil(seq/32)] keep-bit tensor the
// kernel fills when dropout is on (drop_thresh in (0,256); the actual
// drop probability is drop_thresh/256).
void attn_fwd(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor out,
              at::Tensor lse, double scale, bool causal,
              c10::optional<at::Tensor> drop_mask, int64_t seed,
              int64_t drop_thresh, double inv_keep,
              c10::optional<at::Tensor> seqlens) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == at::kBFloat16);
  int64_t in_s[3], o_s[3], tmp[3];
  attn_strides(q, in_s, "q");
  attn_strides(k, tmp, "k");
  TORCH_CHECK(tmp[0] == in_s[0] && tmp[1] == in_s[1] && tmp[2] == in_s[2],
              "q/k/v must share strides");
  attn_strides(v, tmp, "v");
  TORCH_CHECK(tmp[0] == in_s[0] && tmp[1] == in_s[1] && tmp[2] == in_s[2],
              "q/k/v must share strides");
  attn_strides(out, o_s, "out");
  check(lse, at::kFloat, "lse");
  const int64_t heads = q.size(1);
  const int64_t seq = q.size(2);
  const int64_t head_dim = q.size(3);
  const int64_t bh = q.size(0) * heads;
  attn_check_grid(bh, seq, causal);
  unsigned int* mptr = nullptr;
  int64_t mask_w = (seq + 31) / 32;
  if (drop_mask.has_value()) {
    check(*drop_mask, at::kInt, "drop_mask");
    TORCH_CHECK(drop_mask->numel() == bh * seq * mask_w,
                "drop_mask size mismatch");
    TORCH_CHECK(drop_thresh > 0 && drop_thresh < 256, "drop_thresh range");
    mptr = reinterpret_cast<unsigned int*>(drop_mask->data_ptr());
  }
  epl_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(),
               lse.data_ptr<float>(), bh, seq, (float)scale, causal, heads,
               head_dim, in_s, o_s, mptr, mask_w,
               (unsigned long long)seed, (int)drop_thresh,
               (float)inv_keep, attn_seqlens(seqlens, q), cur_stream());
}

void attn_bwd(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor out,
              at::Tensor dout, at::Tensor lse, at::Tensor delta_ws,
              at::Tensor dq, at::Tensor dk, at::Tensor dv, double scale,
              bool causal, bool split_dkdv,
              c10::optional<at::Tensor> drop_mask, double inv_keep,
              c10::optional<at::Tensor> dlse,
              c10::optional<at::Tensor> seqlens) {
  int64_t in_s[3], o_s[3], do_s[3], g_s[3], tmp[3];
  attn_strides(q, in_s, "q");
  attn_strides(out, o_s, "out");
  attn_strides(dout, do_s, "dout");
  attn_strides(dq, g_s, "dq");
  attn_strides(dk, tmp, "dk");
  TORCH_CHECK(tmp[0] == g_s[0] && tmp[1] == g_s[1] && tmp[2] == g_s[2],
              "dq/dk/dv must share strides");
  attn_strides(dv, tmp, "dv");
  TORCH_CHECK(tmp[0] == g_s[0] && tmp[1] == g_s[1] && tmp[2] == g_s[2],
              "dq/dk/dv must share strides");
  const int64_t heads = q.size(1);
  const int64_t seq = q.size(2);
  const int64_t bh = q.size(0) * heads;
  attn_check_grid(bh, seq, causal);
  check(delta_ws, at::kFloat, "delta_ws");
  const unsigned int* mptr = nullptr;
  int64_t mask_w = (seq + 31) / 32;
  if (drop_mask.has_value()) {
    check(*drop_mask, at::kInt, "drop_mask");
    mptr = reinterpret_cast<const unsigned int*>(drop_mask->data_ptr());
  }
  const float* dlse_ptr = nullptr;
  if (dlse.has_value()) {
    check(*dlse, at::kFloat, "dlse");
    TORCH_CHECK(dlse->numel() == bh * seq, "dlse size mismatch");
    dlse_ptr = dlse->data_ptr<float>();
  }
  epl_attn_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(),
               dout.data_ptr(), lse.data_ptr<float>(),
               delta_ws.data_ptr<float>(), dq.data_ptr(), dk.data_ptr(),
               dv.data_ptr(), bh, seq, (float)scale, causal, heads, in_s,
               o_s, do_s, g_s, split_dkdv ? 1 : 0, mptr, mask_w,
               (float)inv_keep, q.size(3), dlse_ptr,
               attn_seqlens(seqlens, q), cur_stream());
}

// out_gather / out_tr: int16 [4 * head_dim/32, 64, 8] (fragment, lane,
// element) — see tr_read_probe_kernel
void tr_read_probe(at::Tensor out_gather, at::Tensor out_tr,
                   int64_t head_dim) {
  TORCH_CHECK(head_dim == 64 || head_dim == 128, "head_dim must be 64|128");
  check(out_gather, at::kShort, "out_gather");
  check(out_tr, at::kShort, "out_tr");
  const int64_t n = 4 * (head_dim / 32) * 64 * 8;
  TORCH_CHECK(out_gather.numel() == n && out_tr.numel() == n,
              "probe outputs must hold ", n, " elements");
  run_tr_read_probe(reinterpret_cast<short*>(out_gather.data_ptr()),
                    reinterpret_cast<short*>(out_tr.data_ptr()),
                    (int)head_dim, cur_stream());
}

// out: int32 [n * bh, 2] — the (bh, blk) of every block of a non-causal
// attention grid dim3(n, bh), at its linear id (block_order_probe_kernel)
void attn_block_order_probe(at::Tensor out, int64_t n, int64_t bh) {
  check(out, at::kInt, "out");
  TORCH_CHECK(n >= 1 && n <= 65535 && bh >= 1 && bh <= 65535,
              "grid dimensions must lie in [1, 65535]");
  TORCH_CHECK(out.numel() == 2 * n * bh, "out must hold ", 2 * n * bh,
              " elements");
  run_block_order_probe(out.data_ptr<int>(), (int)n, (int)bh, cur_stream());
}

// the same map evaluated on the host (no device needed): int32
// [n * bh, 2] on the CPU
at::Tensor attn_block_order_host(int64_t n, int64_t bh) {
  TORCH_CHECK(n >= 1 && n <= 65535 && bh >= 1 && bh <= 65535,
              "grid dimensions must lie in [1, 65535]");
  at::Tensor out = at::empty({n * bh, 2}, at::kInt);
  int* p = out.data_ptr<int>();
  for (int64_t y = 0; y < bh; ++y)
    for (int64_t x = 0; x < n; ++x) {
      const attn_order::Block b = attn_order::block_of(
          (unsigned)x, (unsigned)y, (unsigned)n, (unsigned)bh);
      p[2 * (x + n * y)] = (int)b.bh;
      p[2 * (x + n * y) + 1] = (int)b.blk;
    }
  return out;
}

void mfma_probe(at::Tensor A, at::Tensor B, at::Tensor D) {
  check(A, at::kBFloat16, "A");
  check(B, at::kBFloat16, "B");
  check(D, at::kFloat, "D");
  run_mfma_probe(reinterpret_cast<const unsigned short*>(A.data_ptr()),
                 reinterpret_cast<const unsigned short*>(B.data_ptr()),
                 D.data_ptr<float>(), cur_stream());
}

static void check_idx(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
              t.scalar_type() == at::kLong, name,
              " must be a contiguous int64 device tensor");
}

void moe_dispatch_fwd(at::Tensor disp, at::Tensor x, at::Tensor fe,
                      at::Tensor pos, at::Tensor ft, int64_t cap) {
  check(disp, at::kBFloat16, "disp");
  check(x, at::kBFloat16, "x");
  check_idx(fe, "fe"); check_idx(pos, "pos"); check_idx(ft, "ft");
  const int64_t hidden = x.size(-1);
  TORCH_CHECK(hidden % 8 == 0, "hidden % 8");
  epl_moe_dispatch_fwd(disp.data_ptr(), x.data_ptr(),
                       fe.data_ptr<int64_t>(), pos.data_ptr<int64_t>(),
                       ft.data_ptr<int64_t>(), fe.numel(), hidden, cap,
                       cur_stream());
}

void moe_dispatch_bwd(at::Tensor dx, at::Tensor ddisp, at::Tensor fe,
                      at::Tensor pos, at::Tensor inv, int64_t k,
                      int64_t cap) {
  check(dx, at::kBFloat16, "dx");
  check(ddisp, at::kBFloat16, "ddisp");
  check_idx(fe, "fe"); check_idx(pos, "pos"); check_idx(inv, "inv");
  const int64_t hidden = dx.size(-1);
  epl_moe_dispatch_bwd(dx.data_ptr(), ddisp.data_ptr(),
                       fe.data_ptr<int64_t>(), pos.data_ptr<int64_t>(),
                       inv.data_ptr<int64_t>(), dx.numel() / hidden, k,
                       hidden, cap, cur_stream());
}

void moe_combine_fwd(at::Tensor out, at::Tensor h, at::Tensor fw,
                     at::Tensor fe, at::Tensor pos, at::Tensor inv,
                     int64_t k, int64_t cap) {
  check(out, at::kBFloat16, "out");
  check(h, at::kBFloat16, "h");
  check(fw, at::kFloat, "fw");
  check_idx(fe, "fe"); check_idx(pos, "pos"); check_idx(inv, "inv");
  const int64_t hidden = out.size(-1);
  epl_moe_combine_fwd(out.data_ptr(), h.data_ptr(), fw.data_ptr<float>(),
                      fe.data_ptr<int64_t>(), pos.data_ptr<int64_t>(),
                      inv.data_ptr<int64_t>(), out.numel() / hidden, k,
                      hidden, cap, cur_stream());
}

void moe_combine_bwd(at::Tensor dh, at::Tensor dfw, at::Tensor dout,
                     at::Tensor h, at::Tensor fw, at::Tensor fe,
                     at::Tensor pos, at::Tensor ft, int64_t cap) {
  check(dh, at::kBFloat16, "dh");
  check(dout, at::kBFloat16, "dout");
  check(h, at::kBFloat16, "h");
  check(fw, at::kFloat, "fw");
  check(dfw, at::kFloat, "dfw");
  check_idx(fe, "fe"); check_idx(pos, "pos"); check_idx(ft, "ft");
  const int64_t hidden = dh.size(-1);
  epl_moe_combine_bwd(dh.data_ptr(), dfw.data_ptr<float>(),
                      dout.data_ptr(), h.data_ptr(), fw.data_ptr<float>(),
                      fe.data_ptr<int64_t>(), pos.data_ptr<int64_t>(),
                      ft.data_ptr<int64_t>(), fe.numel(), hidden, cap,
                      cur_stream());
}

static bool aligned16(const at::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

// N tokens, E experts of a [N, E] logits tensor, checked against k
static void router_extents(const at::Tensor& logits, int64_t k, int64_t* n,
                           int64_t* e) {
  TORCH_CHECK(logits.is_cuda() && logits.is_contiguous() &&
              logits.dim() == 2,
              "logits must be a contiguous 2-D device tensor");
  *n = logits.size(0);
  *e = logits.size(1);
  TORCH_CHECK(k == 1 || k == 2, "moe router: k must be 1 or 2, got ", k);
  TORCH_CHECK(*e >= 2 && *e <= 256,
              "moe router: 2 <= num_experts <= 256, got ", *e);
  TORCH_CHECK(*n >= 1 && *n < (int64_t(1) << 30),
              "moe router: 1 <= tokens < 2^30, got ", *n);
}

void moe_router_fwd(at::Tensor logits, int64_t k, at::Tensor topi,
                    at::Tensor topw, at::Tensor lse, at::Tensor counts,
                    at::Tensor psum, at::Tensor losses) {
  const bool bf16 = is_bf16(logits);
  int64_t n, e;
  router_extents(logits, k, &n, &e);
  check_idx(topi, "topi");
  check(topw, at::kFloat, "topw");
  check(lse, at::kFloat, "lse");
  check_idx(counts, "counts");
  check(psum, at::kFloat, "psum");
  check(losses, at::kFloat, "losses");
  TORCH_CHECK(topi.numel() == n * k && topw.numel() == n * k,
              "topi / topw must hold tokens * k elements");
  TORCH_CHECK(lse.numel() == n, "lse must hold one element per token");
  TORCH_CHECK(counts.numel() == e && psum.numel() == e,
              "counts / psum must hold one element per expert");
  TORCH_CHECK(losses.numel() == 2, "losses must hold 2 elements");
  const int64_t waves = epl_moe_router_waves(n, e);
  at::Tensor p_part = at::empty({waves * e + waves},
                                logits.options().dtype(at::kFloat));
  at::Tensor c_part = at::empty({waves * e},
                                logits.options().dtype(at::kInt));
  epl_moe_router_fwd(logits.data_ptr(), topi.data_ptr<int64_t>(),
                     topw.data_ptr<float>(), lse.data_ptr<float>(),
                     counts.data_ptr<int64_t>(), psum.data_ptr<float>(),
                     losses.data_ptr<float>(), p_part.data_ptr<float>(),
                     c_part.data_ptr<int>(), n, e, k, bf16,
                     aligned16(logits), cur_stream());
}

void moe_router_bwd(at::Tensor dlogits, at::Tensor logits, at::Tensor lse,
                    at::Tensor topi, at::Tensor dw, at::Tensor counts,
                    at::Tensor g_bal, at::Tensor g_z, int64_t k) {
  const bool bf16 = is_bf16(logits);
  int64_t n, e;
  router_extents(logits, k, &n, &e);
  check(dlogits, logits.scalar_type(), "dlogits");
  TORCH_CHECK(dlogits.numel() == n * e, "dlogits must match logits");
  check(lse, at::kFloat, "lse");
  check_idx(topi, "topi");
  check(dw, at::kFloat, "dw");
  check_idx(counts, "counts");
  check(g_bal, at::kFloat, "g_bal");
  check(g_z, at::kFloat, "g_z");
  TORCH_CHECK(lse.numel() == n, "lse must hold one element per token");
  TORCH_CHECK(topi.numel() == n * k && dw.numel() == n * k,
              "topi / dw must hold tokens * k elements");
  TORCH_CHECK(counts.numel() == e,
              "counts must hold one element per expert");
  TORCH_CHECK(g_bal.numel() == 1 && g_z.numel() == 1,
              "g_bal / g_z must hold one element");
  epl_moe_router_bwd(dlogits.data_ptr(), logits.data_ptr(),
                     lse.data_ptr<float>(), topi.data_ptr<int64_t>(),
                     dw.data_ptr<float>(), counts.data_ptr<int64_t>(),
                     g_bal.data_ptr<float>(), g_z.data_ptr<float>(), n, e, k,
                     bf16, aligned16(logits) && aligned16(dlogits),
                     cur_stream());
}

void colsum(at::Tensor dy, at::Tensor db, at::Tensor partial) {
  const bool bf16 = is_bf16(dy);
  TORCH_CHECK(dy.is_cuda() && dy.is_contiguous() && dy.dim() == 2,
              "dy must be a contiguous 2-D device tensor");
  const int64_t rows = dy.size(0), cols = dy.size(1);
  TORCH_CHECK(cols % 8 == 0, "cols must be a multiple of 8");
  TORCH_CHECK(db.numel() == cols && db.scalar_type() == dy.scalar_type());
  const int64_t stripes = partial.numel() / cols;
  TORCH_CHECK(stripes >= 1 && partial.scalar_type() == at::kFloat);
  epl_colsum(db.data_ptr(), dy.data_ptr(), partial.data_ptr<float>(), rows,
             cols, stripes, bf16, cur_stream());
}

void sqnorm(at::Tensor t, at::Tensor out) {
  check_arena(t, "t");   // element loads: no alignment beyond the dtype's
  const bool bf16 = is_bf16(t);
  check(out, at::kFloat, "out");
  TORCH_CHECK(out.numel() >= 1, "out must hold one element");
  epl_sqnorm(t.data_ptr(), t.numel(), out.data_ptr<float>(), bf16,
             cur_stream());
}

// ---- LLaMA ops (csrc/kernels/llama_ops.hip) --------------------------------
// Everything a launch relies on is checked here from the tensors' metadata
// alone: no value is read on the host, so the ops stay graph-capturable.

// contiguous bf16 on `dev` with a 16-byte-aligned base
static void check_llama_bf16(const at::Tensor& t, const at::Device& dev,
                             const char* name) {
  check(t, at::kBFloat16, name);
  TORCH_CHECK(t.device() == dev, name, " is on another device");
  TORCH_CHECK(aligned16(t), name, " must be 16-byte aligned");
}

static void check_llama_f32(const at::Tensor& t, const at::Device& dev,
                            int64_t numel, const char* name) {
  check(t, at::kFloat, name);
  TORCH_CHECK(t.device() == dev, name, " is on another device");
  TORCH_CHECK(aligned16(t), name, " must be 16-byte aligned");
  TORCH_CHECK(t.numel() == numel, name, " must hold ", numel, " elements");
}

// rows, cols of a native RMSNorm operand x: bf16, 8 <= cols <= 8192, cols % 8
static void rms_extents(const at::Tensor& x, int64_t* rows, int64_t* cols) {
  TORCH_CHECK(x.dim() >= 1 && x.numel() > 0, "rms_norm: empty input");
  *cols = x.size(-1);
  *rows = x.numel() / *cols;
  TORCH_CHECK(*cols % 8 == 0 && *cols >= 8 && *cols <= 8192,
              "rms_norm: native widths are multiples of 8 up to 8192, got ",
              *cols);
}

// out = s rstd gamma with s = x (+ res), rstd = rsqrt(mean(s^2) + eps);
// with res the summed stream is written to s_out.  rstd: fp32 [rows].
void rms_norm_fwd(at::Tensor out, at::Tensor x, c10::optional<at::Tensor> res,
                  c10::optional<at::Tensor> s_out, at::Tensor gamma,
                  at::Tensor rstd, double eps) {
  int64_t rows, cols;
  const at::Device dev = x.device();
  check_llama_bf16(x, dev, "x");
  rms_extents(x, &rows, &cols);
  check_llama_bf16(out, dev, "out");
  check_llama_bf16(gamma, dev, "gamma");
  TORCH_CHECK(out.numel() == x.numel(), "out must match x");
  TORCH_CHECK(gamma.numel() == cols, "gamma must hold cols elements");
  check_llama_f32(rstd, dev, rows, "rstd");
  TORCH_CHECK(res.has_value() == s_out.has_value(),
              "rms_norm_fwd: res and s come together");
  const void* res_p = nullptr;
  void* s_p = nullptr;
  if (res.has_value()) {
    check_llama_bf16(*res, dev, "res");
    check_llama_bf16(*s_out, dev, "s");
    TORCH_CHECK(res->numel() == x.numel() && s_out->numel() == x.numel(),
                "res and s must match x");
    res_p = res->data_ptr();
    s_p = s_out->data_ptr();
  }
  epl_rms_norm_fwd(out.data_ptr(), x.data_ptr(), res_p, s_p,
                   gamma.data_ptr(), rstd.data_ptr<float>(), rows, cols,
                   (float)eps, cur_stream());
}

// dx = rstd (dy gamma - xhat mean(dy gamma xhat)) (+ dadd), xhat = s rstd;
// dgamma (fp32 [cols], overwritten) = sum_rows dy xhat
void rms_norm_bwd(at::Tensor dx, at::Tensor dgamma, at::Tensor dy,
                  at::Tensor s, at::Tensor gamma, at::Tensor rstd,
                  c10::optional<at::Tensor> dadd) {
  int64_t rows, cols;
  const at::Device dev = s.device();
  check_llama_bf16(s, dev, "s");
  rms_extents(s, &rows, &cols);
  check_llama_bf16(dx, dev, "dx");
  check_llama_bf16(dy, dev, "dy");
  check_llama_bf16(gamma, dev, "gamma");
  TORCH_CHECK(dx.numel() == s.numel() && dy.numel() == s.numel(),
              "dx and dy must match s");
  TORCH_CHECK(gamma.numel() == cols, "gamma must hold cols elements");
  check_llama_f32(dgamma, dev, cols, "dgamma");
  check_llama_f32(rstd, dev, rows, "rstd");
  const void* dadd_p = nullptr;
  if (dadd.has_value()) {
    check_llama_bf16(*dadd, dev, "dadd");
    TORCH_CHECK(dadd->numel() == s.numel(), "dadd must match s");
    dadd_p = dadd->data_ptr();
  }
  const int64_t nparts = epl_rms_norm_bwd_parts(rows, cols);
  at::Tensor ws = at::empty({nparts, cols}, dgamma.options());
  epl_rms_norm_bwd(dx.data_ptr(), dgamma.data_ptr<float>(), dy.data_ptr(),
                   s.data_ptr(), gamma.data_ptr(), rstd.data_ptr<float>(),
                   dadd_p, ws.data_ptr<float>(), rows, cols, cur_stream());
}

// In-place rotary embedding of a [B, S, N, D] view (see rope_kernel):
// rows pos0 .. pos0 + S - 1 of the fp32 [L, D / 2] tables; inverse applies
// the transposed rotation.
void rope_(at::Tensor x, at::Tensor cos_t, at::Tensor sin_t, int64_t pos0,
           bool inverse) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16,
              "rope_: x must be a bf16 device tensor");
  TORCH_CHECK(x.dim() == 4, "rope_: x must be a [B, S, N, D] view");
  const int64_t b = x.size(0), s = x.size(1), n = x.size(2), d = x.size(3);
  TORCH_CHECK(d == 64 || d == 128, "rope_: head_dim must be 64 or 128, got ",
              d);
  TORCH_CHECK(x.stride(3) == 1, "rope_: last dim must be contiguous");
  for (int i = 0; i < 3; ++i)
    TORCH_CHECK(x.size(i) == 1 || (x.stride(i) % 8 == 0 && x.stride(i) >= d),
                "rope_: stride ", i, " must be a multiple of 8 elements "
                "and at least one head, got ", x.stride(i));
  TORCH_CHECK(aligned16(x), "rope_: x must be 16-byte aligned");
  TORCH_CHECK(b * s * n * (d / 16) < (int64_t(1) << 31),
              "rope_: too many elements for one launch");
  const at::Device dev = x.device();
  TORCH_CHECK(cos_t.dim() == 2 && cos_t.size(1) == d / 2,
              "rope_: tables must be [L, D / 2]");
  check_llama_f32(cos_t, dev, cos_t.size(0) * (d / 2), "cos");
  check_llama_f32(sin_t, dev, cos_t.numel(), "sin");
  TORCH_CHECK(pos0 >= 0 && pos0 + s <= cos_t.size(0), "rope_: positions ",
              pos0, " .. ", pos0 + s, " exceed the table length ",
              cos_t.size(0));
  epl_rope(x.data_ptr(), cos_t.data_ptr<float>(), sin_t.data_ptr<float>(),
           x.stride(0), x.stride(1), x.stride(2), b, s, n, d, pos0, inverse,
           cur_stream());
}

// rows, F of a packed [.., 2F] gate/up tensor
static void swiglu_extents(const at::Tensor& gu, int64_t* rows, int64_t* f) {
  TORCH_CHECK(gu.dim() >= 1 && gu.numel() > 0, "swiglu: empty input");
  TORCH_CHECK(gu.size(-1) % 16 == 0, "swiglu: the packed width 2F needs "
              "F % 8 == 0, got ", gu.size(-1));
  *f = gu.size(-1) / 2;
  *rows = gu.numel() / gu.size(-1);
  TORCH_CHECK(*f <= (int64_t(1) << 21), "swiglu: F too large");
}

// out[rows, F] = silu(gu[:, :F]) * gu[:, F:]
void swiglu_fwd(at::Tensor out, at::Tensor gu) {
  int64_t rows, f;
  const at::Device dev = gu.device();
  check_llama_bf16(gu, dev, "gu");
  swiglu_extents(gu, &rows, &f);
  check_llama_bf16(out, dev, "out");
  TORCH_CHECK(out.numel() == rows * f, "out must be [rows, F]");
  epl_swiglu_fwd(out.data_ptr(), gu.data_ptr(), rows, f, cur_stream());
}

// dgu[rows, 2F]: gate half dy u silu'(g), up half dy silu(g)
void swiglu_bwd(at::Tensor dgu, at::Tensor dy, at::Tensor gu) {
  int64_t rows, f;
  const at::Device dev = gu.device();
  check_llama_bf16(gu, dev, "gu");
  swiglu_extents(gu, &rows, &f);
  check_llama_bf16(dgu, dev, "dgu");
  check_llama_bf16(dy, dev, "dy");
  TORCH_CHECK(dgu.numel() == gu.numel(), "dgu must match gu");
  TORCH_CHECK(dy.numel() == rows * f, "dy must be [rows, F]");
  epl_swiglu_bwd(dgu.data_ptr(), dy.data_ptr(), gu.data_ptr(), rows, f,
                 cur_stream());
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "MI355X-native parallel library: RCCL comm core + CDNA4 kernels";
  epl::register_comm(m);
  m.def("fused_adamw", &fused_adamw);
  m.def("colsum", &colsum);
  m.def("lamb_phase1", &lamb_phase1);
  m.def("lamb_phase2", &lamb_phase2);
  m.def("layer_norm_fwd", &layer_norm_fwd);
  m.def("layer_norm_bwd", &layer_norm_bwd);
  m.def("layer_norm_bwd_fused", &layer_norm_bwd_fused, py::arg("dx"),
        py::arg("dgamma"), py::arg("dbeta"), py::arg("dy"), py::arg("x"),
        py::arg("gamma"), py::arg("mean"), py::arg("rstd"),
        py::arg("dadd") = py::none(), py::arg("colsum_out") = py::none());
  m.def("layer_norm_bwd_typed", &layer_norm_bwd_typed, py::arg("dx"),
        py::arg("dgamma"), py::arg("dbeta"), py::arg("dy"), py::arg("x"),
        py::arg("gamma"), py::arg("mean"), py::arg("rstd"),
        py::arg("dadd") = py::none(), py::arg("colsum_out") = py::none(),
        py::arg("dy2") = py::none());
  m.def("bias_gelu_fwd", &bias_gelu_fwd);
  m.def("bias_gelu_bwd", &bias_gelu_bwd);
  m.def("bias_gelu_bwd_typed", &bias_gelu_bwd_typed);
  m.def("ce_rowstats", &ce_rowstats, py::arg("logits"), py::arg("targets"),
        py::arg("row_max"), py::arg("row_sumexp"), py::arg("target_logit"),
        py::arg("vocab_begin"), py::arg("ignore_index"),
        py::arg("skip_ignored") = false);
  m.def("ce_backward", &ce_backward);
  m.def("scale_", &scale_);
  m.def("f32_to_bf16", &f32_to_bf16);
  m.def("bf16_to_f32", &bf16_to_f32);
  m.def("sqnorm", &sqnorm);
  m.def("mfma_probe", &mfma_probe);
  m.def("tr_read_probe", &tr_read_probe);
  m.def("attn_block_order_probe", &attn_block_order_probe);
  m.def("attn_block_order_host", &attn_block_order_host);
  m.def("moe_dispatch_fwd", &moe_dispatch_fwd);
  m.def("moe_dispatch_bwd", &moe_dispatch_bwd);
  m.def("moe_combine_fwd", &moe_combine_fwd);
  m.def("moe_combine_bwd", &moe_combine_bwd);
  m.def("moe_router_fwd", &moe_router_fwd);
  m.def("moe_router_bwd", &moe_router_bwd);
  m.def("moe_router_waves", [](int64_t n, int64_t e) {
    return epl_moe_router_waves(n, e);
  });
  m.def("attn_fwd", &attn_fwd, py::arg("q"), py::arg("k"), py::arg("v"),
        py::arg("out"), py::arg("lse"), py::arg("scale"), py::arg("causal"),
        py::arg("drop_mask"), py::arg("seed"), py::arg("drop_thresh"),
        py::arg("inv_keep"), py::arg("seqlens") = py::none());
  m.def("attn_bwd", &attn_bwd, py::arg("q"), py::arg("k"), py::arg("v"),
        py::arg("out"), py::arg("dout"), py::arg("lse"),
        py::arg("delta_ws"), py::arg("dq"), py::arg("dk"), py::arg("dv"),
        py::arg("scale"), py::arg("causal"), py::arg("split_dkdv"),
        py::arg("drop_mask"), py::arg("inv_keep"), py::arg("dlse"),
        py::arg("seqlens") = py::none());
  m.def("rms_norm_fwd", &rms_norm_fwd, py::arg("out"), py::arg("x"),
        py::arg("res"), py::arg("s"), py::arg("gamma"), py::arg("rstd"),
        py::arg("eps"));
  m.def("rms_norm_bwd", &rms_norm_bwd, py::arg("dx"), py::arg("dgamma"),
        py::arg("dy"), py::arg("s"), py::arg("gamma"), py::arg("rstd"),
        py::arg("dadd") = py::none());
  m.def("rope_", &rope_, py::arg("x"), py::arg("cos"), py::arg("sin"),
        py::arg("pos0"), py::arg("inverse"));
  m.def("swiglu_fwd", &swiglu_fwd);
  m.def("swiglu_bwd", &swiglu_bwd);
}
