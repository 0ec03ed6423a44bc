"""SwiGLU forward / backward (csrc/kernels/llama_ops.hip) against the fp64
reference of llama_refs.py with the derived per-element bounds.

Direct _C.swiglu_fwd / _C.swiglu_bwd calls on inputs from a seeded CPU
generator: randn plus a sweep of the gate over every bf16 value of
[-12, 12], +-40 and +-88 .. +-130 (2^w overflows to inf on one side and the
sigmoid's tail flushes on the other: the results must stay finite).  F
covers one vector, widths that are no multiple of the block, and Llama-2-7B's
11008; 1025 x 4096 needs a second pass of the capped grid.  Every case
asserts

* |got - ref| <= 2 E on out and on both halves of dgu;
* every result is finite;
* every sentinel in the guard rows is untouched: nothing past column 2F of
  the last row, nothing before the first;
* a second run gives the same bits.

``SWIGLU-RATIO`` lines feed the table in docs/testing.md.
"""

import pytest
import torch

from tests import kernel_refs as kr
from tests import llama_refs as lr

pytestmark = pytest.mark.gpu

F64 = torch.float64
BF16 = torch.bfloat16


@pytest.mark.parametrize("rows,f", lr.swiglu_cases())
def test_swiglu_fp64(rows, f):
    from easyparallellibrary_amd import _C
    trouble = []

    def run(inp):
        gu = inp["gu"].to(BF16).cuda()
        dy = inp["dy"].to(BF16).cuda()
        sets = []
        for _ in range(2):
            bufs = {"out": kr.guarded_rows(rows, f, BF16, "cuda"),
                    "dgu": kr.guarded_rows(rows, 2 * f, BF16, "cuda")}
            _C.swiglu_fwd(bufs["out"].view, gu)
            _C.swiglu_bwd(bufs["dgu"].view, dy, gu)
            sets.append(bufs)
        torch.cuda.synchronize()
        for key, buf in sets[0].items():
            if not torch.equal(buf.raw, sets[1][key].raw):
                trouble.append("two runs differ in " + key)
            n = buf.stray_writes()
            if n:
                trouble.append("%d stray writes around %s" % (n, key))
        dgu = sets[0]["dgu"].view.cpu().to(F64)
        return dict(out=sets[0]["out"].view.cpu().to(F64),
                    dgate=dgu[:, :f], dup=dgu[:, f:])

    worst, bad = lr.swiglu_check_case(rows, f, run)
    print("SWIGLU-RATIO rows %d F %d passes %d %s" % (
        rows, f, lr.swiglu_passes(rows, f), lr.format_ratios(worst)))
    assert not bad and not trouble, (bad, trouble)


def test_swiglu_gate_minus_100_is_finite():
    from easyparallellibrary_amd import _C
    gu = torch.cat([torch.full((2, 8), -100.0), torch.full((2, 8), 1.5)],
                   dim=1).to(BF16).cuda()
    dy = torch.ones(2, 8, dtype=BF16, device="cuda")
    out = torch.full((2, 8), float("nan"), dtype=BF16, device="cuda")
    dgu = torch.full((2, 16), float("nan"), dtype=BF16, device="cuda")
    _C.swiglu_fwd(out, gu)
    _C.swiglu_bwd(dgu, dy, gu)
    assert float(out.float().abs().max()) == 0.0
    assert float(dgu.float().abs().max()) == 0.0


def test_swiglu_binding_refuses_and_module_falls_back():
    from easyparallellibrary_amd import _C
    from easyparallellibrary_amd.ops.swiglu import FusedSwiGLU
    gen = torch.Generator().manual_seed(0)
    for dtype, width in ((torch.float32, 64), (BF16, 24)):   # fp32; F = 12
        gu = torch.randn(3, width, generator=gen).to(dtype).cuda()
        out = torch.empty(3, width // 2, dtype=dtype, device="cuda")
        with pytest.raises(RuntimeError):
            _C.swiglu_fwd(out, gu)
        with pytest.raises(RuntimeError):
            _C.swiglu_bwd(torch.empty_like(gu), out, gu)
        x = gu.clone().requires_grad_()
        y = FusedSwiGLU()(x)
        y.float().sum().backward()
        ref = lr.swiglu_ref(gu.cpu().to(F64),
                            torch.ones(3, width // 2, dtype=F64))
        tol = 2.0 ** -7 if dtype == BF16 else 1e-5
        assert bool(((y.detach().cpu().to(F64) - ref["out"]).abs()
                     <= tol * (1 + ref["out"].abs())).all())
        assert bool(torch.isfinite(x.grad).all())
    with pytest.raises(RuntimeError):                        # out too small
        _C.swiglu_fwd(torch.empty(3, 8, dtype=BF16, device="cuda"),
                      torch.zeros(4, 16, dtype=BF16, device="cuda"))
