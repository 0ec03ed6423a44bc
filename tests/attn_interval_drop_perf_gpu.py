"""Interval attention with dropout, timings (not a pytest file; run it on
the GPU):

    python tests/attn_interval_drop_perf_gpu.py [--out FILE]

One process, the sides alternating, median / minimum / spread (max - min)
of 5 x 50 calls after 10 warm-up calls, host clock around a device
synchronise, as attn_interval_perf_gpu.py.  Forward (no_grad) and forward
+ backward at b128 H16 d64 s512 with 4 documents per row and at b8 H32
Hkv8 d128 s2048 with 8, p = 0.1:

  drop    ``interval_attention(dropout_p=0.1)``: the dropout kernels
  nodrop  ``interval_attention()``: what the PRNG and the mask words cost
  sdpa    ``_masked_sdpa`` with the dense boolean mask of the same bounds
          and dropout_p = 0.1 on K / V expanded to H heads: the route
          dropout took before these kernels"""

import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# H, Hkv, d, s, b, documents per row
SHAPES = [(16, 16, 64, 512, 128, 4), (32, 8, 128, 2048, 8, 8)]
P = 0.1


def measure(fns, reps=5, calls=50):
    """{name: (median, min, max - min) us}; the functions alternate per
    repetition"""
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
    return {name: (sorted(v)[len(v) // 2], min(v), max(v) - min(v))
            for name, v in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import easyparallellibrary_amd as epl
    from easyparallellibrary_amd.ops.attention import (
        _masked_sdpa, interval_attention, interval_bounds)
    epl.init()
    log = []
    for h, hkv, d, s, b, ndocs in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(11)
        q, dout = (torch.randn(b, h, s, d, device="cuda",
                               dtype=torch.bfloat16, generator=gen)
                   for _ in range(2))
        k, v = (torch.randn(b, hkv, s, d, device="cuda",
                            dtype=torch.bfloat16, generator=gen)
                for _ in range(2))
        leaves = [t.requires_grad_() for t in (q, k, v)]
        pos = torch.arange(s, device="cuda")
        bounds = interval_bounds((pos // (s // ndocs))[None].repeat(b, 1),
                                 None, s, "cuda")

        def sdpa():
            return _masked_sdpa(q, k.repeat_interleave(h // hkv, dim=1),
                                v.repeat_interleave(h // hkv, dim=1), False,
                                d ** -0.5, P, None, bounds[0], bounds[1])

        sides = {
            "drop": lambda: interval_attention(q, k, v, bounds, dropout_p=P),
            "nodrop": lambda: interval_attention(q, k, v, bounds),
            "sdpa": sdpa}

        def fwd(f):
            def run():
                with torch.no_grad():
                    f()
            return run

        def fwd_bwd(f):
            def run():
                for t in leaves:
                    t.grad = None
                f().backward(dout)
            return run

        for kind, wrap in (("fwd", fwd), ("f+b", fwd_bwd)):
            res = measure({n: wrap(f) for n, f in sides.items()})
            for n, (med, lo, spread) in res.items():
                line = ("b{} H{} Hkv{} s{} d{} docs{} p{} {} {}: {:.1f} us "
                        "(min {:.1f}, spread {:.1f})  {:.3f} of nodrop, "
                        "{:.3f} of sdpa").format(
                            b, h, hkv, s, d, ndocs, P, n, kind, med, lo,
                            spread, med / res["nodrop"][0],
                            med / res["sdpa"][0])
                print(line, flush=True)
                log.append(line)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(log) + "\n")


if __name__ == "__main__":
    main()
