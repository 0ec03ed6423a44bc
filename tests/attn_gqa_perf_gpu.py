"""Grouped-query flash attention timings (not a pytest file; run it on the
GPU):

    python tests/attn_gqa_perf_gpu.py [--out FILE] [--variant NAME=PATH ...]

Native GQA (``flash_attention`` with Hkv < H kv heads) against what a caller
had to do before on the same build: ``repeat_interleave`` on K and V into
the MHA kernels, autograd summing dk / dv.  Forward (no_grad) and forward +
backward, same process, the two alternating, median and minimum of 5 x 50
calls after 10 warm-up calls, host clock around a device synchronise.

``--variant NAME=PATH`` adds another build of the extension (a _C*.so made
from csrc/kernels/attention_gqa.hip with a define): each runs the native
path in a child process, this build and the variants alternating, two
rounds, in the same session.  The defines:

    -DEPL_ATTN_GQA_PLAIN_ORDER  causal q-parallel grids keep bh = blockIdx.x
    -DEPL_ATTN_GQA_DK_PIPELINED d64 non-causal dK pipelined like dV

``--counters [--ext PATH]`` runs 20 forward calls of the first causal shape
and nothing else: the process to put under a counter-only profiler run
(TCC_EA0_RDREQ_sum), once per build.  profiles/attn_gqa_ab.txt keeps one
run."""

import argparse
import importlib.util
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# H, Hkv, d, s, causal, b
SHAPES = [(32, 8, 128, 4096, True, 2),
          (32, 8, 128, 2048, True, 8),
          (16, 4, 64, 512, False, 128)]


def load_ext(path):
    """this build's extension, or another build's in its place"""
    import torch  # noqa: F401  (the extension links against it)
    import easyparallellibrary_amd
    if path:
        spec = importlib.util.spec_from_file_location(
            "easyparallellibrary_amd._C", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        sys.modules["easyparallellibrary_amd._C"] = mod
        easyparallellibrary_amd._C = mod


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


def make(shape):
    import torch
    from easyparallellibrary_amd.ops.attention import flash_attention
    h, hkv, d, s, causal, b = shape
    gen = torch.Generator(device="cuda").manual_seed(11)
    q, dout = (torch.randn(b, h, s, d, device="cuda", dtype=torch.bfloat16,
                           generator=gen) for _ in range(2))
    k, v = (torch.randn(b, hkv, s, d, device="cuda", dtype=torch.bfloat16,
                        generator=gen) for _ in range(2))
    leaves = [t.requires_grad_() for t in (q, k, v)]

    def native():
        return flash_attention(q, k, v, causal=causal)

    def expand():
        return flash_attention(q, k.repeat_interleave(h // hkv, dim=1),
                               v.repeat_interleave(h // hkv, dim=1),
                               causal=causal)

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
    return native, expand, fwd, fwd_bwd


def label(shape):
    h, hkv, d, s, causal, b = shape
    return "b{} H{} Hkv{} s{} d{} {}".format(
        b, h, hkv, s, d, "causal" if causal else "full")


def worker(name, ext, native_only):
    load_ext(ext)
    import torch
    import easyparallellibrary_amd as epl
    epl.init()
    order = name
    for shape in SHAPES:
        native, expand, fwd, fwd_bwd = make(shape)
        fns = {"native fwd": fwd(native), "native f+b": fwd_bwd(native)}
        if not native_only:
            fns.update({"expand fwd": fwd(expand),
                        "expand f+b": fwd_bwd(expand)})
        for name, (med, lo) in measure(fns).items():
            print("[{}] {} {}: {:.1f} us (min {:.1f})".format(
                order, label(shape), name, med, lo), flush=True)
        torch.cuda.empty_cache()


def counters(ext):
    load_ext(ext)
    import torch
    import easyparallellibrary_amd as epl
    epl.init()
    native, _, fwd, _ = make(SHAPES[0])
    for _ in range(20):
        fwd(native)()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--variant", action="append", default=[])
    ap.add_argument("--worker", default=None)
    ap.add_argument("--ext", default=None)
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--counters", action="store_true")
    args = ap.parse_args()
    if args.counters:
        return counters(args.ext)
    if args.worker:
        return worker(args.worker, args.ext, args.native_only)
    variants = [v.split("=", 1) for v in args.variant]
    runs = [("this build", None, False)]
    for _ in range(2):
        for name, path in variants:
            runs += [(name, os.path.abspath(path), True),
                     ("this build", None, True)]
    log = []
    for name, path, native_only in runs:
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", name]
        if path:
            cmd += ["--ext", path]
        if native_only:
            cmd.append("--native-only")
        # a failed child ends the session: nothing more starts on the GPU
        res = subprocess.run(cmd, cwd=REPO, stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True,
                             timeout=400)
        text = "\n".join(line for line in res.stdout.splitlines()
                         if line.startswith("["))
        print(text, flush=True)
        log.append(text)
        if res.returncode != 0:
            print(res.stdout[-3000:])
            sys.exit(res.returncode)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(log) + "\n")


if __name__ == "__main__":
    main()
