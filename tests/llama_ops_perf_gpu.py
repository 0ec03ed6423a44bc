"""A/B of the LLaMA kernels against the torch compositions they replace
(run by hand on an MI355X; output kept in profiles/llama_ops_ab.txt).

Shapes: rows 16384 (b8 x s2048), hidden 2048 / 4096, F 5632 / 11008,
H32 d128 for RoPE.  Per op the native kernel and the torch composition
alternate inside the same call; reported is the median of 5 timings of 50
calls each, the bytes the op has to move (from the shapes) and TB/s.  Then
one LlamaBlock forward + backward, native against kernel.fused off.
No GPU work happens at import.
"""

import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS = 16384
BATCH, SEQ = 8, 2048
EPS = 1e-5
# the project's measured streaming kernels, as the yardstick
YARDSTICK = "yardstick: LayerNorm fwd 6.05 TB/s, bias-GeLU 5.4 TB/s"


def _time_us(fn, calls=50):
    import torch
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def ab(label, native, composed, nbytes, reps=5, calls=50):
    import torch
    for _ in range(5):
        native()
        composed()
    torch.cuda.synchronize()
    nat, com = [], []
    for _ in range(reps):
        nat.append(_time_us(native, calls))
        com.append(_time_us(composed, calls))
    nat.sort()
    com.sort()
    n, c = nat[reps // 2], com[reps // 2]
    print("%-34s native %8.1f us %5.2f TB/s | torch %8.1f us %5.2f TB/s | "
          "x%.2f" % (label, n, nbytes / n / 1e6, c, nbytes / c / 1e6, c / n),
          flush=True)


def rms_ops(cols):
    import torch
    from easyparallellibrary_amd import _C
    bf = torch.bfloat16
    x = torch.randn(ROWS, cols, device="cuda", dtype=bf)
    res = torch.randn_like(x)
    g = torch.randn(cols, device="cuda", dtype=bf)
    dy = torch.randn_like(x)
    out, s, dx = (torch.empty_like(x) for _ in range(3))
    rstd = torch.empty(ROWS, dtype=torch.float32, device="cuda")
    dg = torch.empty(cols, dtype=torch.float32, device="cuda")
    one = ROWS * cols * 2

    def comp(xv, gv):
        xf = xv.float()
        return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + EPS)
                * gv.float()).to(bf)

    ab("rms_norm fwd h%d" % cols,
       lambda: _C.rms_norm_fwd(out, x, None, None, g, rstd, EPS),
       lambda: comp(x, g), 2 * one)
    ab("rms_norm fwd+res h%d" % cols,
       lambda: _C.rms_norm_fwd(out, x, res, s, g, rstd, EPS),
       lambda: comp(x + res, g), 4 * one)
    _C.rms_norm_fwd(out, x, res, s, g, rstd, EPS)
    xr = x.clone().requires_grad_()
    gr = g.clone().requires_grad_()

    def comp_fb():
        xr.grad = gr.grad = None
        comp(xr, gr).backward(dy)

    def nat_fb():
        _C.rms_norm_fwd(out, x, None, None, g, rstd, EPS)
        _C.rms_norm_bwd(dx, dg, dy, x, g, rstd, None)

    ab("rms_norm fwd+bwd h%d" % cols, nat_fb, comp_fb, 5 * one)
    ab("rms_norm bwd (vs torch f+b) h%d" % cols,
       lambda: _C.rms_norm_bwd(dx, dg, dy, s, g, rstd, None), comp_fb,
       3 * one)
    ab("rms_norm bwd+dadd (same) h%d" % cols,
       lambda: _C.rms_norm_bwd(dx, dg, dy, s, g, rstd, res), comp_fb,
       4 * one)


def rope_ops(heads=32, d=128):
    import torch
    from easyparallellibrary_amd import _C
    from easyparallellibrary_amd.ops.rope import rope_tables
    bf = torch.bfloat16
    qkv = torch.randn(BATCH, SEQ, 3, heads, d, device="cuda", dtype=bf)
    cos, sin = rope_tables("cuda", d, 10000.0, SEQ)
    view = qkv[:, :, :2].view(BATCH, SEQ, 2 * heads, d)
    c16 = torch.cat([cos[:SEQ], cos[:SEQ]], -1).to(bf)[None, :, None, :]
    s16 = torch.cat([sin[:SEQ], sin[:SEQ]], -1).to(bf)[None, :, None, :]

    def hf(t):
        half = d // 2
        rot = torch.cat([-t[..., half:], t[..., :half]], dim=-1)
        return t * c16 + rot * s16

    def composed():
        q, k, _ = qkv.unbind(dim=2)
        return hf(q), hf(k)

    ab("rope q,k in packed qkv h%d d%d" % (heads, d),
       lambda: _C.rope_(view, cos, sin, 0, False), composed,
       BATCH * SEQ * 2 * heads * d * 2 * 2)


def swiglu_ops(f):
    import torch
    import torch.nn.functional as F
    from easyparallellibrary_amd import _C
    bf = torch.bfloat16
    gu = torch.randn(ROWS, 2 * f, device="cuda", dtype=bf)
    dy = torch.randn(ROWS, f, device="cuda", dtype=bf)
    out = torch.empty(ROWS, f, device="cuda", dtype=bf)
    dgu = torch.empty_like(gu)
    one = ROWS * f * 2

    def comp(t):
        g, u = t.chunk(2, dim=-1)
        return F.silu(g) * u

    ab("swiglu fwd F%d" % f, lambda: _C.swiglu_fwd(out, gu),
       lambda: comp(gu), 3 * one)
    gr = gu.clone().requires_grad_()

    def comp_fb():
        gr.grad = None
        comp(gr).backward(dy)

    def nat_fb():
        _C.swiglu_fwd(out, gu)
        _C.swiglu_bwd(dgu, dy, gu)

    ab("swiglu fwd+bwd F%d" % f, nat_fb, comp_fb, 8 * one)
    ab("swiglu bwd (vs torch f+b) F%d" % f,
       lambda: _C.swiglu_bwd(dgu, dy, gu), comp_fb, 5 * one)


def block_ab(hidden=4096, heads=32, ffn=11008):
    import torch
    import easyparallellibrary_amd as epl
    from easyparallellibrary_amd.models.llama import LlamaBlock
    torch.manual_seed(0)
    block = LlamaBlock(hidden, heads, ffn).to("cuda", torch.bfloat16)
    x = torch.randn(BATCH, SEQ, hidden, device="cuda",
                    dtype=torch.bfloat16).requires_grad_()
    dy = torch.randn(BATCH, SEQ, hidden, device="cuda", dtype=torch.bfloat16)

    def step():
        x.grad = None
        block.zero_grad(set_to_none=True)
        block(x).backward(dy)

    res = {}
    for fused in (True, False, True, False):
        epl.init(epl.Config({"kernel.fused": fused}))
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        res.setdefault(fused, []).extend(
            _time_us(step, calls=5) for _ in range(3))
    nat = sorted(res[True])[len(res[True]) // 2]
    tor = sorted(res[False])[len(res[False]) // 2]
    print("LlamaBlock h%d H%d F%d b%d s%d fwd+bwd: native %.0f us | "
          "kernel.fused off %.0f us | x%.3f" % (
              hidden, heads, ffn, BATCH, SEQ, nat, tor, tor / nat),
          flush=True)


def main():
    import torch
    import easyparallellibrary_amd as epl
    assert torch.cuda.is_available(), "needs a GPU"
    epl.init()
    print(YARDSTICK)
    print("rows %d (b%d x s%d); median of 5 x 50 calls, native and torch "
          "alternating" % (ROWS, BATCH, SEQ))
    for cols in (2048, 4096):
        rms_ops(cols)
    rope_ops()
    for f in (5632, 11008):
        swiglu_ops(f)
    block_ab()


if __name__ == "__main__":
    main()
