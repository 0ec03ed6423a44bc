"""Flash attention forward + backward timings for the per-sample-length
change (not a pytest file; run it on the GPU):

* the dense path must not pay: f+b without seqlens at the two shapes of
  tests/attn_perf_gpu.py (the causal one with dropout too), this build
  against another build of the
  extension (``--parent-ext path/to/_C*.so``, e.g. the parent commit's),
  fresh processes, the two builds alternating;
* what the lengths buy: b128 h16 s512 d64 non-causal f+b, dense, seqlens
  all 512, and lengths drawn uniformly from [64, 512] with a fixed seed,
  with sum(len^2) / (B seq^2) of that draw.

Direct _C calls on preallocated buffers (the positional signature both
builds share), median and minimum of 5 x 50 calls after 10 warm-up calls,
host clock around a device synchronise.  profiles/attn_varlen_ab.txt keeps
one run."""

import argparse
import importlib.util
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = [(128, 16, 512, False), (16, 25, 1024, True)]
D = 64


def load_ext(path):
    import torch  # noqa: F401  (the extension links against it)
    import easyparallellibrary_amd
    if path is None:
        from easyparallellibrary_amd import _C
        return _C
    spec = importlib.util.spec_from_file_location(
        "easyparallellibrary_amd._C", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sys.modules["easyparallellibrary_amd._C"] = mod
    easyparallellibrary_amd._C = mod
    return mod


def timed(fn, label, reps=5, calls=50):
    import torch
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) / calls * 1e6)
    us.sort()
    print("{}: {:.1f} us  (min {:.1f} us over {} x {} calls)".format(
        label, us[len(us) // 2], us[0], reps, calls), flush=True)
    return us[len(us) // 2]


def make_fb(ext, b, h, s, causal, seqlens=None, thresh=0):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(1)
    q, k, v, dout = (torch.randn(b, h, s, D, device="cuda", generator=gen)
                     .to(torch.bfloat16) for _ in range(4))
    out = torch.empty(b, s, h, D, dtype=torch.bfloat16,
                      device="cuda").permute(0, 2, 1, 3)
    lse = torch.empty(b * h * s, dtype=torch.float32, device="cuda")
    delta = torch.empty_like(lse)
    dq, dk, dv = (torch.empty_like(q) for _ in range(3))
    scale = D ** -0.5
    tail = () if seqlens is None else (seqlens,)
    mask = torch.empty(b * h * s * ((s + 31) // 32), dtype=torch.int32,
                       device="cuda") if thresh else None
    inv_keep = 256.0 / (256 - thresh)

    def fb():
        ext.attn_fwd(q, k, v, out, lse, scale, causal, mask, 12345, thresh,
                     inv_keep, *tail)
        ext.attn_bwd(q, k, v, out, dout, lse, delta, dq, dk, dv, scale,
                     causal, True, mask, inv_keep, None, *tail)
    return fb


def child(ext_path, varlen):
    import torch
    ext = load_ext(ext_path)
    for b, h, s, causal in SHAPES:
        timed(make_fb(ext, b, h, s, causal),
              "dense f+b b{} h{} s{} causal={}".format(b, h, s, causal))
    # the dropout kernels with direct staging (causal d64) are the
    # instantiations whose register allocation moved most
    b, h, s, causal = SHAPES[1]
    timed(make_fb(ext, b, h, s, causal, thresh=26),
          "dense f+b b{} h{} s{} causal={} dropout 26/256".format(
              b, h, s, causal))
    if not varlen:
        return
    b, h, s = 128, 16, 512
    dense = timed(make_fb(ext, b, h, s, False), "varlen-shape dense f+b")
    full = torch.full((b,), s, dtype=torch.int32, device="cuda")
    t_full = timed(make_fb(ext, b, h, s, False, full),
                   "varlen-shape seqlens all {} f+b".format(s))
    gen = torch.Generator().manual_seed(2024)
    lens = torch.randint(64, s + 1, (b,), generator=gen)
    ratio = float((lens.double() ** 2).sum() / (b * s * s))
    t_mixed = timed(make_fb(ext, b, h, s, False, lens.int().cuda()),
                    "varlen-shape lengths U[64,{}] seed 2024 f+b".format(s))
    print("  sum(len^2)/(B seq^2) = {:.4f}, mean len {:.1f}; all-{} / dense "
          "= {:.4f}, mixed / dense = {:.4f}".format(
              ratio, float(lens.double().mean()), s, t_full / dense,
              t_mixed / dense), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-ext", default=None,
                    help="another build of the extension to alternate with")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--ext", default=None)
    ap.add_argument("--no-varlen", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args.ext, not args.no_varlen)
        return
    for i in range(1, args.rounds + 1):
        builds = [("new", None)]
        if args.parent_ext:
            builds.insert(0, ("parent", os.path.abspath(args.parent_ext)))
        for name, ext in builds:
            print("## perf_{}_{}".format(name, i), flush=True)
            cmd = [sys.executable, os.path.abspath(__file__), "--child"]
            if ext:
                cmd += ["--ext", ext, "--no-varlen"]
            # a child that fails ends the run: nothing more starts on the GPU
            subprocess.run(cmd, cwd=REPO, check=True, timeout=240)


if __name__ == "__main__":
    main()
