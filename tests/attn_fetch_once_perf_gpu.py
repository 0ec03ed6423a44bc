"""Flash attention forward and backward timings for the XCD-local block
order and the combined dK+dV kernel, this build against other builds of
the extension (not a pytest file; run it on the GPU):

    python tests/attn_fetch_once_perf_gpu.py --parent-ext path/to/_C*.so \
        [--variant NAME=PATH,SPLIT ...]

Direct _C.attn_fwd / _C.attn_bwd calls on preallocated buffers in the
qkv-strided layout of the BERT step ([B,S,3,H,D] projection buffer, out
and dout in [B,S,H,D] order), a fresh process per block, the variants
alternating, median and minimum of 5 x 50 calls after 10 warm-up calls,
host clock around a device synchronise, two rounds.

Variants: ``parent`` (--parent-ext, split kernels), ``split`` (this build,
split_dkdv=True: the block order alone), ``new`` (this build,
split_dkdv=False: block order + combined kernel).  ``--variant`` adds a
further build with its split flag (SPLIT = 0 or 1), e.g. a build with the
identity block order to time the combined kernel alone.

Shapes: the BERT-Large one (b128 h16 s512 d64, non-causal), the same with
lengths drawn from U[64, 512], seed 2024, and two causal shapes (b16 h25
s1024 d64, b32 h16 s1024 d128) whose kernels and grids the change does not
touch: they are the controls and count as unmoved inside 2 %.
profiles/attn_fetch_once_ab.txt keeps one run."""

import argparse
import importlib.util
import os
import re
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# label, b, h, s, d, causal, lengths, control
CASES = [
    ("b128 h16 s512 d64 full", 128, 16, 512, 64, False, False, False),
    ("b128 h16 s512 d64 full lengths U[64,512] seed 2024", 128, 16, 512, 64,
     False, True, False),
    ("b16 h25 s1024 d64 causal", 16, 25, 1024, 64, True, False, True),
    ("b32 h16 s1024 d128 causal", 32, 16, 1024, 128, True, False, True),
]


def load_ext(path):
    import torch  # noqa: F401  (the extension links against it)
    import easyparallellibrary_amd
    if not path:
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


def make_calls(ext, split, b, h, s, d, causal, lengths):
    """(fwd, bwd) closures on one set of buffers"""
    import torch
    gen = torch.Generator(device="cuda").manual_seed(1)
    qkv = torch.randn(b, s, 3, h, d, device="cuda",
                      generator=gen).to(torch.bfloat16)
    q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
    out = torch.empty(b, s, h, d, dtype=torch.bfloat16,
                      device="cuda").permute(0, 2, 1, 3)
    dout = torch.randn(b, s, h, d, device="cuda", generator=gen).to(
        torch.bfloat16).permute(0, 2, 1, 3)
    dqkv = torch.empty_like(qkv)
    dq, dk, dv = (dqkv[:, :, i].transpose(1, 2) for i in range(3))
    lse = torch.empty(b * h * s, dtype=torch.float32, device="cuda")
    delta = torch.empty_like(lse)
    tail = ()
    if lengths:
        lg = torch.Generator().manual_seed(2024)
        tail = (torch.randint(64, s + 1, (b,), generator=lg).int().cuda(),)
    scale = d ** -0.5

    def fwd():
        ext.attn_fwd(q, k, v, out, lse, scale, causal, None, 0, 0, 1.0,
                     *tail)

    def bwd():
        ext.attn_bwd(q, k, v, out, dout, lse, delta, dq, dk, dv, scale,
                     causal, split, None, 1.0, None, *tail)
    return fwd, bwd


def child(ext_path, split):
    ext = load_ext(ext_path)
    for label, b, h, s, d, causal, lengths, _ in CASES:
        fwd, bwd = make_calls(ext, split, b, h, s, d, causal, lengths)
        timed(fwd, "fwd " + label)   # leaves the out and lse bwd reads
        timed(bwd, "bwd " + label)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-ext", default=None,
                    help="the parent commit's build of the extension")
    ap.add_argument("--variant", action="append", default=[],
                    metavar="NAME=PATH,SPLIT",
                    help="a further build and its split flag (repeatable)")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--child-ext", default="")
    ap.add_argument("--child-split", type=int, default=1)
    args = ap.parse_args()
    if args.child:
        child(args.child_ext, bool(args.child_split))
        return
    variants = []
    if args.parent_ext:
        variants.append(("parent", os.path.abspath(args.parent_ext), 1))
    variants += [("split", "", 1), ("new", "", 0)]
    for item in args.variant:
        name, rest = item.split("=", 1)
        path, split = rest.rsplit(",", 1)
        variants.append((name, os.path.abspath(path), int(split)))
    med = {}
    for i in range(1, args.rounds + 1):
        for name, ext, split in variants:
            print("## fetch_once_perf_{}_{}".format(name, i), flush=True)
            cmd = [sys.executable, os.path.abspath(__file__), "--child",
                   "--child-ext", ext, "--child-split", str(split)]
            # a child that fails ends the run: nothing more starts on the GPU
            res = subprocess.run(cmd, cwd=REPO, check=True, timeout=300,
                                 stdout=subprocess.PIPE, text=True)
            sys.stdout.write(res.stdout)
            sys.stdout.flush()
            for line in res.stdout.splitlines():
                hit = re.match(r"((?:fwd|bwd) .*): ([0-9.]+) us", line)
                if hit:
                    med.setdefault(hit.group(1), {}).setdefault(
                        name, []).append(float(hit.group(2)))
    print("## summary (median over rounds of the per-round medians, us)")
    base = variants[0][0]
    moved = []
    for label, *_, control in CASES:
        for kind in ("fwd", "bwd"):
            key = "{} {}".format(kind, label)
            row = {n: statistics.median(v) for n, v in med[key].items()}
            text = "  ".join("{} {:.1f}".format(n, row[n])
                             for n, _, _ in variants)
            text += "  " + "  ".join(
                "{}/{} {:.4f}".format(n, base, row[n] / row[base])
                for n, _, _ in variants if n != base)
            print("{}: {}".format(key, text))
            if control:
                moved += [(key, n) for n, _, _ in variants
                          if abs(row[n] / row[base] - 1.0) > 0.02]
    print("controls: {}".format(
        "unmoved (all within 2 % of {})".format(base) if not moved
        else "MOVED by more than 2 %: {}".format(moved)))


if __name__ == "__main__":
    main()
