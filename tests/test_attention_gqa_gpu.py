"""Grouped-query flash attention (csrc/kernels/attention_gqa.hip): direct
_C.attn_fwd_gqa / _C.attn_bwd_gqa calls against the fp64 reference of
kernel_refs.py on k and v expanded with repeat_interleave.

The expanded reference's dk, dv and their per-head bounds are summed over
each group: the kernels add a group's fp32 contributions and round once,
so the sum of the per-head bounds bounds them (triangle inequality).
delta is checked against attn_delta_ref on the kernel's own bf16 out, as
in test_attention_fp64_gpu.py.  Every case runs twice and asks for equal
bits: the group sum has one writer and a fixed order.
"""

import pytest
import torch

from tests import attn_group_cases as gc
from tests import kernel_refs as kr

pytestmark = pytest.mark.gpu

F64 = torch.float64
BF16 = torch.bfloat16
GRADS = ("out", "dq", "dk", "dv")


def gqa_inputs(family, seq, d, causal, hkv, b=2, h=6):
    """the joint families of attn_group_cases.py under the dense mask"""
    return gc.group_inputs(family, seq, d, h, hkv, b,
                           gc.dense_valid(seq, b, causal))


def gqa_ref(q, k, v, dout, causal):
    """(ref, bounds) with dk / dv and their bounds summed per group"""
    b, h, seq, d = q.shape
    hkv = k.shape[1]
    scale = d ** -0.5
    ke, ve = (t.repeat_interleave(h // hkv, dim=1) for t in (k, v))
    ref = kr.attn_ref(q, ke, ve, dout, causal, scale)
    bounds = kr.attn_bounds(ref, q, ke, ve, dout, scale)
    for name in ("dk", "dv"):
        ref[name] = ref[name].view(b, hkv, h // hkv, seq, d).sum(2)
        bounds[name] = bounds[name].view(b, hkv, h // hkv, seq, d).sum(2)
    return ref, bounds


def gqa_run(q, k, v, dout, causal, layout, seqlens=None):
    """one forward + backward on the GPU; results on the CPU"""
    from easyparallellibrary_amd import _C
    b, h, seq, d = q.shape
    hkv = k.shape[1]
    dev = "cuda"
    if layout == "packed":
        def packed():
            buf = torch.full((b, seq, h + 2 * hkv, d), float("nan"),
                             dtype=BF16, device=dev)
            return (buf[:, :, :h].transpose(1, 2),
                    buf[:, :, h:h + hkv].transpose(1, 2),
                    buf[:, :, h + hkv:].transpose(1, 2))
        tq, tk, tv = packed()
        dq, dk, dv = packed()
    else:
        tq, dq = (torch.empty(b, h, seq, d, dtype=BF16, device=dev)
                  for _ in range(2))
        tk, tv, dk, dv = (torch.empty(b, hkv, seq, d, dtype=BF16, device=dev)
                          for _ in range(4))
    for dst, src in ((tq, q), (tk, k), (tv, v)):
        dst.copy_(src.to(BF16))
    for t in (dq, dk, dv):
        t.fill_(float("nan"))
    tdo = dout.to(BF16).to(dev)
    out = torch.full((b, seq, h, d), float("nan"), dtype=BF16,
                     device=dev).permute(0, 2, 1, 3)
    lse = torch.full((b * h * seq,), float("nan"), device=dev)
    delta = torch.full((b * h * seq,), float("nan"), device=dev)
    sl = None if seqlens is None else torch.tensor(
        seqlens, dtype=torch.int32, device=dev)
    scale = d ** -0.5
    _C.attn_fwd_gqa(tq, tk, tv, out, lse, scale, causal, sl)
    _C.attn_bwd_gqa(tq, tk, tv, out, tdo, lse, delta, dq, dk, dv, scale,
                    causal, sl)
    torch.cuda.synchronize()
    res = dict(out=out.cpu(), dq=dq.cpu(), dk=dk.cpu(), dv=dv.cpu(),
               lse=lse.cpu().view(b, h, seq), delta=delta.cpu().view(b, h, seq))
    return res


def check(res, ref, bounds, dout, rows=slice(None)):
    """every output finite and inside its bound on ``rows``"""
    got = {n: t.to(F64)[:, :, rows] for n, t in res.items()}
    for name in kr.ATTN_OUTPUTS:
        want, bound = ref[name], bounds[name]
        if name == "delta":
            want, bound = kr.attn_delta_ref(dout, got["out"])
        assert bool(torch.isfinite(got[name]).all()), name
        ratio = kr.attn_ratio((got[name] - want).abs(), bound)
        print("GQA-RATIO {} {:.3f}".format(name, ratio))
        assert ratio <= kr.ATTN_FACTOR[name], (name, ratio)


def same_bits(a, b):
    for name in a:
        assert torch.equal(a[name].view(torch.int16 if a[name].dtype == BF16
                                        else torch.int32),
                           b[name].view(torch.int16 if b[name].dtype == BF16
                                        else torch.int32)), name


CASES = [(seq, "randn") for seq in (72, 200, 257)] + [(200, "peaked")]


@pytest.mark.parametrize("layout", ["plain", "packed"])
@pytest.mark.parametrize("seq,family", CASES)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("hkv", [3, 2, 1])
def test_gqa_against_fp64(hkv, d, causal, seq, family, layout):
    inp = gqa_inputs(family, seq, d, causal, hkv)
    ref, bounds = gqa_ref(*inp, causal)
    res = gqa_run(*inp, causal, layout)
    check(res, ref, bounds, inp[3])
    same_bits(res, gqa_run(*inp, causal, layout))


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_gqa_seqlens(d, causal):
    """lengths [0, 130] at seq 200: padded rows are exact zeros, valid rows
    match the reference taken on the truncated sample"""
    seq, lens = 200, [0, 130]
    inp = gqa_inputs("randn", seq, d, causal, 2)
    res = gqa_run(*inp, causal, "plain", seqlens=lens)
    for name in GRADS:
        for b, n in enumerate(lens):
            assert not bool(res[name][b, :, n:].to(F64).abs().any()), name
    cut = [t[1:, :, :130] for t in inp]
    ref, bounds = gqa_ref(*cut, causal)
    check({n: t[1:] for n, t in res.items()}, ref, bounds, cut[3],
          rows=slice(0, 130))
    same_bits(res, gqa_run(*inp, causal, "plain", seqlens=lens))


@pytest.mark.parametrize("d,causal", [(64, False), (64, True)])
def test_gqa_permuted_block_order(d, causal):
    """B * Hkv = 16: the permuted branch of both group-aware orders runs"""
    inp = gqa_inputs("randn", 257, d, causal, 2, b=8, h=4)
    ref, bounds = gqa_ref(*inp, causal)
    check(gqa_run(*inp, causal, "plain"), ref, bounds, inp[3])
