"""A/B of the dropout-add-LN kernels at the BERT-Large site shape (run by
hand on an MI355X; output kept in profiles/ln_dropout_ab.txt).

65536 x 1024 bf16 (b128 x s512), a post-LN site: y = LN(D(x) + res), fp32
LN parameters, every call through FusedLayerNorm, forward alone (no grad)
and forward + backward.  Three sides alternate inside one process:

  (a) dropout_p = 0.1 in the LN kernels, lin_bias given (the fused site);
  (b) F.dropout(x, 0.1) then today's fused LN: the composition (a)
      replaces.  Without lin_bias, whose gradient (b) would have to reduce
      separately: (b) is flattered by that missing reduction;
  (c) today's fused LN with no dropout, lin_bias given: (a) - (c) is the
      cost of the philox work and of the second gradient tensor.

Reported: the median of 5 timings of 20 calls each, and (a)/(b), (a)/(c).
Then the stand-alone dropout_add against F.dropout + add.  No GPU work
happens at import.
"""

import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS, COLS, P = 65536, 1024, 0.1


def _time_us(fn, calls=20):
    import torch
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def abc(label, sides, reps=5):
    import torch
    for _ in range(3):
        for fn in sides:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in sides]
    for _ in range(reps):
        for t, fn in zip(times, sides):
            t.append(_time_us(fn))
    med = [sorted(t)[reps // 2] for t in times]
    print("%-22s " % label + " | ".join(
        "(%s) %8.1f us" % (n, m) for n, m in zip("abc", med)) +
        " | " + "  ".join("(a)/(%s) %.3f" % (n, med[0] / m)
                          for n, m in zip("bc", med[1:])), flush=True)


def main():
    import torch
    import torch.nn.functional as F
    import easyparallellibrary_amd as epl
    from easyparallellibrary_amd.ops.layer_norm import (FusedLayerNorm,
                                                        dropout_add)
    assert torch.cuda.is_available(), "needs a GPU"
    epl.init()
    torch.manual_seed(0)
    bf = torch.bfloat16
    ln = FusedLayerNorm(COLS).cuda().train()
    x = torch.randn(ROWS, COLS, device="cuda", dtype=bf).requires_grad_()
    res = torch.randn(ROWS, COLS, device="cuda", dtype=bf).requires_grad_()
    dy = torch.randn(ROWS, COLS, device="cuda", dtype=bf)
    lb = torch.zeros(COLS, device="cuda", requires_grad=True)
    print("%d x %d bf16, p = %.1f; median of 5 x 20 calls, sides "
          "alternating" % (ROWS, COLS, P))
    calls = (lambda: ln(x, residual=res, lin_bias=lb, dropout_p=P),
             lambda: ln(F.dropout(x, P, True), residual=res),
             lambda: ln(x, residual=res, lin_bias=lb))

    def fwd(call):
        def run():
            with torch.no_grad():
                call()
        return run

    def fwd_bwd(call):
        def run():
            x.grad = res.grad = lb.grad = None
            ln.zero_grad(set_to_none=True)
            call().backward(dy)
        return run

    abc("LN site fwd", [fwd(c) for c in calls])
    abc("LN site fwd+bwd", [fwd_bwd(c) for c in calls])

    def add_fb(call):
        def run():
            x.grad = res.grad = None
            call().backward(dy)
        return run

    adds = (lambda: dropout_add(x, res, P),
            lambda: res + F.dropout(x, P, True))
    abc("dropout_add fwd", [fwd(c) for c in adds])
    abc("dropout_add fwd+bwd", [add_fb(c) for c in adds])


if __name__ == "__main__":
    main()
