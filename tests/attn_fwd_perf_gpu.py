"""Flash attention FORWARD timings, this build against other builds of the
extension (not a pytest file; run it on the GPU):

    python tests/attn_fwd_perf_gpu.py --parent-ext path/to/_C*.so

Forward only, direct _C.attn_fwd calls on preallocated buffers, a fresh
process per block, the builds alternating (parent, new, parent, new, ...),
median and minimum of 5 x 50 calls after 10 warm-up calls, host clock
around a device synchronise.  ``--ext name=path`` (repeatable) adds further
builds to the rotation, e.g. one per compile-time variant while a kernel
change is being decided.

Shapes: the BERT-Large one (b128 h16 s512 d64, non-causal), the GPT-2 one
(b16 h25 s1024 d64 causal, with and without dropout 26/256), one d128
shape, and the BERT shape with lengths drawn from U[64, 512], seed 2024.
The last line of a run with --parent-ext gives new / parent per shape from
the medians over the rounds; the project counts 2 % as noise.
profiles/attn_fwd_lean_ab.txt keeps one run."""

import argparse
import importlib.util
import os
import re
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# label, b, h, s, d, causal, dropout threshold, lengths
CASES = [
    ("b128 h16 s512 d64 full", 128, 16, 512, 64, False, 0, False),
    ("b16 h25 s1024 d64 causal", 16, 25, 1024, 64, True, 0, False),
    ("b16 h25 s1024 d64 causal dropout 26/256", 16, 25, 1024, 64, True, 26,
     False),
    ("b32 h16 s1024 d128 causal", 32, 16, 1024, 128, True, 0, False),
    ("b128 h16 s512 d64 full lengths U[64,512] seed 2024", 128, 16, 512, 64,
     False, 0, True),
]


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


def make_fwd(ext, b, h, s, d, causal, thresh, lengths):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(1)
    q, k, v = (torch.randn(b, h, s, d, device="cuda", generator=gen)
               .to(torch.bfloat16) for _ in range(3))
    out = torch.empty(b, s, h, d, dtype=torch.bfloat16,
                      device="cuda").permute(0, 2, 1, 3)
    lse = torch.empty(b * h * s, dtype=torch.float32, device="cuda")
    mask = torch.empty(b * h * s * ((s + 31) // 32), dtype=torch.int32,
                       device="cuda") if thresh else None
    tail = ()
    if lengths:
        lg = torch.Generator().manual_seed(2024)
        tail = (torch.randint(64, s + 1, (b,), generator=lg).int().cuda(),)
    scale = d ** -0.5
    inv_keep = 256.0 / (256 - thresh)

    def fwd():
        ext.attn_fwd(q, k, v, out, lse, scale, causal, mask, 12345, thresh,
                     inv_keep, *tail)
    return fwd


def child(ext_path):
    ext = load_ext(ext_path)
    for label, *case in CASES:
        timed(make_fwd(ext, *case), "fwd " + label)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-ext", default=None,
                    help="another build of the extension to alternate with")
    ap.add_argument("--ext", action="append", default=[],
                    metavar="NAME=PATH", help="a further build (repeatable)")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--child-ext", default=None)
    args = ap.parse_args()
    if args.child:
        child(args.child_ext)
        return
    builds = []
    if args.parent_ext:
        builds.append(("parent", os.path.abspath(args.parent_ext)))
    builds.append(("new", None))
    for item in args.ext:
        name, path = item.split("=", 1)
        builds.append((name, os.path.abspath(path)))
    med = {}
    for i in range(1, args.rounds + 1):
        for name, ext in builds:
            print("## fwd_perf_{}_{}".format(name, i), flush=True)
            cmd = [sys.executable, os.path.abspath(__file__), "--child"]
            if ext:
                cmd += ["--child-ext", ext]
            # a child that fails ends the run: nothing more starts on the GPU
            res = subprocess.run(cmd, cwd=REPO, check=True, timeout=240,
                                 stdout=subprocess.PIPE, text=True)
            sys.stdout.write(res.stdout)
            sys.stdout.flush()
            for line in res.stdout.splitlines():
                hit = re.match(r"fwd (.*): ([0-9.]+) us", line)
                if hit:
                    med.setdefault(hit.group(1), {}).setdefault(
                        name, []).append(float(hit.group(2)))
    print("## summary (median over rounds of the per-round medians, us)")
    worst = 0.0
    for label, *_ in CASES:
        row = {n: sorted(v)[len(v) // 2] for n, v in med[label].items()}
        text = "  ".join("{} {:.1f}".format(n, row[n]) for n, _ in builds)
        if "parent" in row:
            text += "  " + "  ".join(
                "{}/parent {:.4f}".format(n, row[n] / row["parent"])
                for n, _ in builds if n != "parent")
            worst = max(worst, row["new"] / row["parent"])
        print("{}: {}".format(label, text))
    if args.parent_ext:
        print("worst new/parent {:.4f} ({})".format(
            worst, "within 2 %" if worst <= 1.02 else "SLOWER than 2 %"))
        sys.exit(0 if worst <= 1.02 else 1)


if __name__ == "__main__":
    main()
