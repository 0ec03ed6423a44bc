"""In-place RoPE kernel (csrc/kernels/llama_ops.hip: rope_kernel) against
the fp64 reference of llama_refs.py with the derived per-element bound.

Direct _C.rope_ calls on seeded CPU inputs in guarded buffers, B = 2, H = 3,
for every layout the op feeds the kernel:

* packed : the q and k slices of a [B, S, 3, H, D] buffer as one
           [B, S, 2H, D] view; the v slice must keep its exact bits;
* bhsd   : a stand-alone [B, H, S, D] tensor (the view is its transpose);
* bshd   : a stand-alone [B, S, H, D] tensor;
* padded : head, token and batch strides with gaps, at a storage offset;
           the gaps hold sentinels that must survive.

Every case runs the forward and then the inverse on the same buffer and
asserts |got - ref| <= 2 E for both, that inverse-after-forward returns the
input within the propagated bound, finiteness, untouched guards, and that
two runs give the same bits.  ``ROPE-RATIO`` lines feed docs/testing.md.
"""

import pytest
import torch

from tests import kernel_refs as kr
from tests import llama_refs as lr

pytestmark = pytest.mark.gpu

F64 = torch.float64
BF16 = torch.bfloat16
B, H = lr.ROPE_B, lr.ROPE_H


def _layout(name, seq, d):
    """(GuardedBuffer, kernel view [B, S, N, D], rotated heads N, view of
    the part that must keep its bits or None)"""
    guard = 2 * (d + 16)
    if name == "packed":
        buf = kr.GuardedBuffer(
            (B, seq, 3, H, d),
            (seq * 3 * H * d, 3 * H * d, H * d, d, 1), 0, BF16, "cuda", guard)
        return (buf, buf.view[:, :, :2].view(B, seq, 2 * H, d), 2 * H,
                buf.view[:, :, 2])
    if name == "bhsd":
        buf = kr.GuardedBuffer((B, H, seq, d), (H * seq * d, seq * d, d, 1),
                               0, BF16, "cuda", guard)
        return buf, buf.view.transpose(1, 2), H, None
    if name == "bshd":
        buf = kr.GuardedBuffer((B, seq, H, d), (seq * H * d, H * d, d, 1),
                               0, BF16, "cuda", guard)
        return buf, buf.view, H, None
    assert name == "padded"
    sn = d + 8
    ss = H * sn + 16
    sb = seq * ss + 8
    buf = kr.GuardedBuffer((B, seq, H, d), (sb, ss, sn, 1), 8, BF16, "cuda",
                           guard)
    return buf, buf.view, H, None


@pytest.mark.parametrize("layout", lr.ROPE_LAYOUTS)
@pytest.mark.parametrize("d,seq,pos0", lr.rope_cases())
def test_rope_fp64(d, seq, pos0, layout):
    from easyparallellibrary_amd import _C
    from easyparallellibrary_amd.ops.rope import rope_tables
    cos, sin = rope_tables("cuda", d, lr.ROPE_THETA, 4000 + 257)
    cos_c, sin_c = cos.cpu(), sin.cpu()
    rc, rs = lr.rope_tables_ref(d, lr.ROPE_THETA, cos.shape[0])
    assert torch.equal(cos_c, rc) and torch.equal(sin_c, rs)
    bad = []
    runs = []
    for _ in range(2):
        buf, view, n, keep = _layout(layout, seq, d)
        x = lr.rope_input(seq, d, n)
        view.copy_(x.to(BF16))
        keep_in = None
        if keep is not None:
            keep.copy_(lr.rope_input(seq, d, H, seed=5).to(BF16))
            keep_in = keep.clone()
        _C.rope_(view, cos, sin, pos0, False)
        fwd_bits = buf.raw.clone()
        got_y = view.cpu().to(F64)
        _C.rope_(view, cos, sin, pos0, True)
        torch.cuda.synchronize()
        runs.append((fwd_bits, buf.raw.clone()))
    if not (torch.equal(runs[0][0], runs[1][0]) and
            torch.equal(runs[0][1], runs[1][1])):
        bad.append("two runs differ")
    if buf.stray_writes():
        bad.append("%d stray writes" % buf.stray_writes())
    if keep is not None and not torch.equal(keep.view(torch.int16),
                                            keep_in.view(torch.int16)):
        bad.append("the v slice changed")
    back = view.cpu().to(F64)
    y, m = lr.rope_ref(x, cos_c, sin_c, pos0)
    e_y = lr.rope_bounds(y, m)
    r_fwd = lr.ratio_of(got_y, y, e_y)
    # the inverse at the forward's own result
    yi, mi = lr.rope_ref(got_y, cos_c, sin_c, pos0, inverse=True)
    e_i = lr.rope_bounds(yi, mi)
    r_inv = lr.ratio_of(back, yi, e_i)
    # round trip: the forward's allowed error 2 E_y goes through the
    # rotation as |c| e1 + |s| e2 (resp. |c| e2 + |s| e1)
    half = d // 2
    c = cos_c[pos0:pos0 + seq].to(F64)[None, :, None, :].abs()
    s = sin_c[pos0:pos0 + seq].to(F64)[None, :, None, :].abs()
    e1, e2 = 2 * e_y[..., :half], 2 * e_y[..., half:]
    carried = torch.cat([c * e1 + s * e2, c * e2 + s * e1], dim=-1)
    # the exact inverse of the exact forward is x up to cos^2 + sin^2 of
    # the fp32 tables: 2^-22 relative
    r_rt = lr.ratio_of(back, x, 2 * e_i + carried + 2.0 ** -22 * mi)
    print("ROPE-RATIO d %d seq %d pos0 %d %s fwd=%.3f inv=%.3f roundtrip=%.3f"
          % (d, seq, pos0, layout, r_fwd, r_inv, r_rt))
    for name, r, lim in (("forward", r_fwd, 2.0), ("inverse", r_inv, 2.0),
                         ("round trip", r_rt, 1.0)):
        if not r <= lim:
            bad.append("%s err/E %.3g > %g" % (name, r, lim))
    if not (bool(torch.isfinite(got_y).all()) and
            bool(torch.isfinite(back).all())):
        bad.append("not finite")
    assert not bad, bad


def test_rope_binding_refuses():
    from easyparallellibrary_amd import _C
    from easyparallellibrary_amd.ops.rope import rope_tables
    cos, sin = rope_tables("cuda", 64, lr.ROPE_THETA, 2048)
    length = cos.shape[0]
    x = torch.zeros(2, 8, 3, 64, dtype=BF16, device="cuda")
    _C.rope_(x, cos, sin, length - 8, False)        # the last rows: fine
    with pytest.raises(RuntimeError):
        _C.rope_(x, cos, sin, length - 7, False)    # one past the table
    with pytest.raises(RuntimeError):
        _C.rope_(x, cos, sin, -1, False)
    with pytest.raises(RuntimeError):               # head_dim 96
        _C.rope_(torch.zeros(2, 8, 3, 96, dtype=BF16, device="cuda"),
                 *rope_tables("cuda", 96, lr.ROPE_THETA, 2048), 0, False)
    flat = torch.zeros(2 * 8 * 3 * 64 + 64, dtype=BF16, device="cuda")
    with pytest.raises(RuntimeError):               # base not 16-byte aligned
        _C.rope_(flat[4:4 + x.numel()].view(2, 8, 3, 64), cos, sin, 0, False)
    with pytest.raises(RuntimeError):               # head stride 68
        _C.rope_(torch.zeros(2, 8, 3, 68, dtype=BF16,
                             device="cuda")[..., :64], cos, sin, 0, False)
    with pytest.raises(RuntimeError):               # fp32 data
        _C.rope_(x.float(), cos, sin, 0, False)
    with pytest.raises(RuntimeError):               # bf16 tables
        _C.rope_(x, cos.to(BF16), sin.to(BF16), 0, False)
    torch.cuda.synchronize()
    assert float(x.float().abs().max()) == 0.0
