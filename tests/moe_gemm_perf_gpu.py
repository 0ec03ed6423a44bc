"""Expert FFN timings: the grouped GEMM kernels against the torch.bmm path
(not a pytest file; run it on the GPU):

    python tests/moe_gemm_perf_gpu.py [--out FILE]

The bench layer's shape (8 experts, capacity 2560, hidden 1024, ffn 4096),
the expert FFN alone: forward (no_grad) and forward + backward.  Native is
``_GroupedExpertLinear`` (two nn, two nt, two tn launches, GeLU in the
epilogues); bmm is what ExpertParallelMLP runs otherwise, GeLU and the
w2^T copy of its backward included.  Fills: every row live, half of every
expert's rows live, and the counts that the layer's own gate gives at
initialisation for 8192 random tokens, top-2, capacity factor 1.25.  Dead
rows hold zeros, as after the dispatch.  One process, the two paths
alternating, median and minimum of 5 x 50 calls after 10 warm-up calls of
every shape, host clock around a device synchronise.  TFLOP/s counts the
live rows only (2 * 2 * live * hidden * ffn per forward, three times that
with the backward), for both paths.

End to end, in the same session, each step under its own time limit:

    EPL_MOE_NATIVE_GEMM=0 timeout 300 python bench.py --config moe \\
        --gpus 1 --steps 20 --warmup 5 && \\
    EPL_MOE_NATIVE_GEMM=1 timeout 300 python bench.py --config moe ... && \\
    (the pair once more)

profiles/moe_gemm_ab.txt keeps one run of both."""

import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

E, CAP, HIDDEN, FFN, TOP_K = 8, 2560, 1024, 4096, 2


def measure(fns, reps=5, calls=50):
    """{name: (median us, min us)}; the functions alternate per repetition"""
    import torch
    for fn in fns.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) / calls * 1e6)
    return {name: (sorted(v)[len(v) // 2], min(v)) for name, v in us.items()}


def router_rows():
    """live rows per expert from the layer's gate at initialisation"""
    import torch
    from easyparallellibrary_amd.ops.moe import ExpertParallelMLP
    torch.manual_seed(0)
    m = ExpertParallelMLP(HIDDEN, 64, E, top_k=TOP_K).to("cuda",
                                                         torch.bfloat16)
    n = int(CAP * E / (1.25 * TOP_K))
    x = torch.randn(n, HIDDEN, device="cuda", dtype=torch.bfloat16)
    with torch.no_grad():
        topi = m.gate(x).float().softmax(-1).topk(TOP_K, dim=-1).indices
    return torch.bincount(topi.reshape(-1), minlength=E).clamp(max=CAP)


def make(rows):
    import torch
    import torch.nn.functional as F
    from easyparallellibrary_amd.ops.moe import (_BatchedExpertLinear,
                                                 _GroupedExpertLinear)
    gen = torch.Generator(device="cuda").manual_seed(5)

    def rand(*shape, std=1.0):
        return (torch.randn(*shape, device="cuda", generator=gen) *
                std).to(torch.bfloat16)
    x, dh = rand(E, CAP, HIDDEN), rand(E, CAP, HIDDEN)
    dead = torch.arange(CAP, device="cuda")[None, :] >= rows[:, None]
    x[dead] = 0
    dh[dead] = 0
    w1, w2 = rand(E, HIDDEN, FFN, std=0.02), rand(E, FFN, HIDDEN, std=0.02)
    leaves = [t.requires_grad_() for t in (x, w1, w2)]
    rows32 = rows.to(torch.int32)

    def native():
        return _GroupedExpertLinear.apply(x, w1, w2, rows32)

    def bmm():
        he = F.gelu(_BatchedExpertLinear.apply(x, w1))
        return _BatchedExpertLinear.apply(he, w2)

    def fwd(f):
        def run():
            with torch.no_grad():
                f()
        return run

    def fwd_bwd(f):
        def run():
            for t in leaves:
                t.grad = None
            f().backward(dh)
        return run
    return {"native fwd": fwd(native), "bmm fwd": fwd(bmm),
            "native f+b": fwd_bwd(native), "bmm f+b": fwd_bwd(bmm)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import easyparallellibrary_amd as epl
    epl.init()
    full = torch.full((E,), CAP, device="cuda")
    fills = [("fill 1.0", full), ("fill 0.5", full // 2),
             ("router fill", router_rows())]
    log = []
    for label, rows in fills:
        live = int(rows.sum())
        head = "{}: rows {} ({:.3f} of {})".format(
            label, rows.tolist(), live / (E * CAP), E * CAP)
        print(head, flush=True)
        log.append(head)
        for name, (med, lo) in measure(make(rows)).items():
            flop = 4.0 * live * HIDDEN * FFN * (3 if "f+b" in name else 1)
            line = "  {}: {:.1f} us (min {:.1f}), {:.1f} TFLOP/s".format(
                name, med, lo, flop / med / 1e6)
            print(line, flush=True)
            log.append(line)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(log) + "\n")


if __name__ == "__main__":
    main()
