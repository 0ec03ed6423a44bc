// Interval flash attention for gfx950 with in-kernel philox dropout: the
// DROP = true instantiations of attn_interval.h (design notes there) and
// their launches.  The forward fills `mask`, int32 [B * H, seq, mask_w]
// keep bits (bit kv & 31 of word kv >> 5 of row q), for the sub-tiles it
// visits; the backward reads it.

#include "attn_interval.h"

extern "C" {

void epl_attn_fwd_interval_drop(const void* q, const void* k, const void* v,
                                void* out, float* lse, int64_t batch_heads,
                                int64_t seq, float scale, int64_t heads,
                                int64_t kv_heads, int64_t head_dim,
                                const int64_t* in_strides,
                                const int64_t* kv_strides,
                                const int64_t* o_strides, const int* seqlens,
                                const int* kv_lo, const int* kv_hi,
                                int64_t bound_sb, unsigned int* mask,
                                int64_t mask_w, unsigned long long seed,
                                int thresh, float inv_keep,
                                hipStream_t stream) {
  const IntervalDrop<true> da = {mask, mask_w, (unsigned int)seed,
                                 (unsigned int)(seed >> 32), thresh,
                                 inv_keep};
  launch_fwd_interval<true>(q, k, v, out, lse, batch_heads, seq, scale,
                            heads, kv_heads, head_dim, in_strides,
                            kv_strides, o_strides, seqlens, kv_lo, kv_hi,
                            bound_sb, da, stream);
}

void epl_attn_bwd_interval_drop(
    const void* q, const void* k, const void* v, const void* out,
    const void* dout, const float* lse, float* delta_ws, void* dq, void* dk,
    void* dv, int64_t batch_heads, int64_t seq, float scale, int64_t heads,
    int64_t kv_heads, int64_t head_dim, const int64_t* in_strides,
    const int64_t* kv_strides, const int64_t* o_strides,
    const int64_t* do_strides, const int64_t* g_strides,
    const int64_t* gkv_strides, const int* seqlens, const int* kv_lo,
    const int* kv_hi, const int* q_lo, const int* q_hi, int64_t bound_sb,
    const unsigned int* mask, int64_t mask_w, float inv_keep,
    hipStream_t stream) {
  // the backward only reads the words; seed and threshold are the
  // forward's business
  const IntervalDrop<true> da = {const_cast<unsigned int*>(mask), mask_w,
                                 0u, 0u, 0, inv_keep};
  launch_bwd_interval<true>(q, k, v, out, dout, lse, delta_ws, dq, dk, dv,
                            batch_heads, seq, scale, heads, kv_heads,
                            head_dim, in_strides, kv_strides, o_strides,
                            do_strides, g_strides, gkv_strides, seqlens,
                            kv_lo, kv_hi, q_lo, q_hi, bound_sb, da, stream);
}

}  // extern "C"
