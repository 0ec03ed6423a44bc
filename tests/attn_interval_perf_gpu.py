"""Interval flash attention timings (not a pytest file; run it on the GPU):

    python tests/attn_interval_perf_gpu.py [--out FILE]

One process, the sides of a comparison alternating, median and minimum of
5 x 50 calls after 10 warm-up calls, host clock around a device
synchronise.  Forward (no_grad) and forward + backward at the BERT shape
b128 H16 d64 s512 (docs4, docs8, win128) and at b8 H32 Hkv8 d128 s2048
(docs8, win512):

  dense    today's non-causal ``flash_attention`` call
  trivial  bounds 0 and S through the interval kernels: the price of the
           path
  docsN    N equal documents per row
  winW     window |i - j| < W
  sdpa-*   scaled_dot_product_attention with the dense boolean mask of the
           same bounds on K / V expanded to H heads: the path that served
           these cases before (BERT shape only)

Next to each banded case the fraction of the dense call's 64-key forward
tiles (per 128-row block) that the interval kernels visit is printed: the
ratio to compare their times with."""

import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# H, Hkv, d, s, b, documents per row, window, with the SDPA sides
SHAPES = [(16, 16, 64, 512, 128, (4, 8), 128, True),
          (32, 8, 128, 2048, 8, (8,), 512, False)]


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


def tile_fraction(kv_lo, kv_hi, s):
    """64-key tiles a forward block of 128 rows visits under the bounds
    over those of the dense call"""
    seen = full = 0
    for q0 in range(0, s, 128):
        last = min(q0 + 128, s) - 1
        seen += (int(kv_hi[last]) - (int(kv_lo[q0]) & ~63) + 63) // 64
        full += (s + 63) // 64
    return seen / full


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    import easyparallellibrary_amd as epl
    from easyparallellibrary_amd.ops.attention import (
        flash_attention, interval_attention, interval_bounds)
    epl.init()
    log = []
    for h, hkv, d, s, b, ndocs, window, with_sdpa in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(11)
        q, dout = (torch.randn(b, h, s, d, device="cuda",
                               dtype=torch.bfloat16, generator=gen)
                   for _ in range(2))
        k, v = (torch.randn(b, hkv, s, d, device="cuda",
                            dtype=torch.bfloat16, generator=gen)
                for _ in range(2))
        leaves = [t.requires_grad_() for t in (q, k, v)]
        pos = torch.arange(s, device="cuda")
        cases = {"trivial": interval_bounds(None, None, s, "cuda")}
        for n in ndocs:
            cases["docs{}".format(n)] = interval_bounds(
                (pos // (s // n))[None].repeat(b, 1), None, s, "cuda")
        cases["win{}".format(window)] = interval_bounds(None, window, s,
                                                        "cuda")
        masks = {}
        if with_sdpa:
            masks = {n: ((pos >= bd[0][:, None, :, None])
                         & (pos < bd[1][:, None, :, None]))
                     for n, bd in cases.items() if n != "trivial"}

        def native(bounds):
            if bounds is None:
                return lambda: flash_attention(q, k, v)
            return lambda: interval_attention(q, k, v, bounds)

        def sdpa(mask):
            return lambda: F.scaled_dot_product_attention(
                q, k.repeat_interleave(h // hkv, dim=1),
                v.repeat_interleave(h // hkv, dim=1), attn_mask=mask)

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

        sides = {"dense": native(None)}
        sides.update({n: native(bd) for n, bd in cases.items()})
        sides.update({"sdpa-" + n: sdpa(m) for n, m in masks.items()})
        for kind, wrap in (("fwd", fwd), ("f+b", fwd_bwd)):
            res = measure({n: wrap(f) for n, f in sides.items()})
            for n, (med, lo) in res.items():
                frac = ""
                if n in cases:
                    frac = "  tiles {:.3f}  time {:.3f} of dense".format(
                        tile_fraction(cases[n][0][0].tolist(),
                                      cases[n][1][0].tolist(), s),
                        med / res["dense"][0])
                line = "b{} H{} Hkv{} s{} d{} {} {}: {:.1f} us (min {:.1f}){}" \
                    .format(b, h, hkv, s, d, n, kind, med, lo, frac)
                print(line, flush=True)
                log.append(line)
        del masks, sides
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(log) + "\n")


if __name__ == "__main__":
    main()
