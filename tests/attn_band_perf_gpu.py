"""Banded causal flash attention timings (not a pytest file; run it on the
GPU):

    python tests/attn_band_perf_gpu.py [--out FILE]

One process, the sides of a comparison alternating, median and minimum of
5 x 50 calls after 10 warm-up calls, host clock around a device
synchronise.  Forward (no_grad) and forward + backward of
``flash_attention`` at b8 H32 Hkv8 s2048 d128 and b2 H32 Hkv8 s4096 d128:

  causal   today's causal GQA call (no band arguments)
  trivial  one document and window >= S through the band kernels: the cost
           of the extra bounds
  docs8    eight equal documents per row
  win512   window = 512
  sdpa-*   scaled_dot_product_attention with the dense boolean mask of the
           same band on K / V expanded to H heads: the path that served
           the two cases before

Next to docs8 / win512 the fraction of the causal call's 64-key tiles
(per 128-row block) that the band visits is printed: the ratio to compare
their times with."""

import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# H, Hkv, d, s, b
SHAPES = [(32, 8, 128, 2048, 8), (32, 8, 128, 4096, 2)]


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


def tile_fraction(kv_lo, s):
    """64-key tiles a forward block of 128 rows visits under the band over
    those of the plain causal call"""
    band = full = 0
    for q0 in range(0, s, 128):
        end = min(q0 + 128, s)
        band += (end - (int(kv_lo[q0]) & ~63) + 63) // 64
        full += (end + 63) // 64
    return band / full


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    import easyparallellibrary_amd as epl
    from easyparallellibrary_amd.ops.attention import (
        band_bounds, flash_attention)
    epl.init()
    log = []
    for h, hkv, d, s, b in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(11)
        q, dout = (torch.randn(b, h, s, d, device="cuda",
                               dtype=torch.bfloat16, generator=gen)
                   for _ in range(2))
        k, v = (torch.randn(b, hkv, s, d, device="cuda",
                            dtype=torch.bfloat16, generator=gen)
                for _ in range(2))
        leaves = [t.requires_grad_() for t in (q, k, v)]
        docs = (torch.arange(s, device="cuda") // (s // 8))[None].repeat(b, 1)
        bands = {"trivial": band_bounds(torch.zeros_like(docs), s, s, "cuda"),
                 "docs8": band_bounds(docs, None, s, "cuda"),
                 "win512": band_bounds(None, 512, s, "cuda")}
        pos = torch.arange(s, device="cuda")
        masks = {n: ((pos[None, :] <= pos[:, None])
                     & (pos >= bands[n][0][:, None, :, None]))
                 for n in ("docs8", "win512")}

        def native(bounds):
            return lambda: flash_attention(q, k, v, causal=True,
                                           bounds=bounds)

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

        sides = {"causal": native(None)}
        sides.update({n: native(bd) for n, bd in bands.items()})
        sides.update({"sdpa-" + n: sdpa(m) for n, m in masks.items()})
        for kind, wrap in (("fwd", fwd), ("f+b", fwd_bwd)):
            res = measure({n: wrap(f) for n, f in sides.items()})
            for n, (med, lo) in res.items():
                frac = ""
                if n in masks:
                    frac = "  tiles {:.3f}  time {:.3f} of causal".format(
                        tile_fraction(bands[n][0][0].tolist(), s),
                        med / res["causal"][0])
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
