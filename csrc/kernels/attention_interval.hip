// Interval flash attention for gfx950, the no-dropout instantiations:
// the kernel templates, their design notes and the host launches are in
// attn_interval.h.  A translation unit of its own, so that the MHA, GQA
// and band instantiations compile to the code they compiled to before
// these kernels existed; the dropout forms are in
// attention_interval_drop.hip for the same reason.

#include "attn_interval.h"

extern "C" {

void epl_attn_fwd_interval(const void* q, const void* k, const void* v,
                           void* out, float* lse, int64_t batch_heads,
                           int64_t seq, float scale, int64_t heads,
                           int64_t kv_heads, int64_t head_dim,
                           const int64_t* in_strides,
                           const int64_t* kv_strides,
                           const int64_t* o_strides, const int* seqlens,
                           const int* kv_lo, const int* kv_hi,
                           int64_t bound_sb, hipStream_t stream) {
  launch_fwd_interval<false>(q, k, v, out, lse, batch_heads, seq, scale,
                             heads, kv_heads, head_dim, in_strides,
                             kv_strides, o_strides, seqlens, kv_lo, kv_hi,
                             bound_sb, IntervalDrop<false>{}, stream);
}

void epl_attn_bwd_interval(const void* q, const void* k, const void* v,
                           const void* out, const void* dout,
                           const float* lse, float* delta_ws, void* dq,
                           void* dk, void* dv, int64_t batch_heads,
                           int64_t seq, float scale, int64_t heads,
                           int64_t kv_heads, int64_t head_dim,
                           const int64_t* in_strides,
                           const int64_t* kv_strides,
                           const int64_t* o_strides,
                           const int64_t* do_strides,
                           const int64_t* g_strides,
                           const int64_t* gkv_strides, const int* seqlens,
                           const int* kv_lo, const int* kv_hi,
                           const int* q_lo, const int* q_hi,
                           int64_t bound_sb, hipStream_t stream) {
  launch_bwd_interval<false>(q, k, v, out, dout, lse, delta_ws, dq, dk, dv,
                             batch_heads, seq, scale, heads, kv_heads,
                             head_dim, in_strides, kv_strides, o_strides,
                             do_strides, g_strides, gkv_strides, seqlens,
                             kv_lo, kv_hi, q_lo, q_hi, bound_sb,
                             IntervalDrop<false>{}, stream);
}

}  // extern "C"
