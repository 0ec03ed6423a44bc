import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import easyparallellibrary_amd as epl
epl.init()
from easyparallellibrary_amd import _C

rows, cols = 65536, 1024
x = torch.randn(rows, cols, device="cuda", dtype=torch.bfloat16)
g = torch.randn(cols, device="cuda", dtype=torch.bfloat16)
b = torch.randn(cols, device="cuda", dtype=torch.bfloat16)
dy = torch.randn_like(x)
mean = torch.empty(rows, dtype=torch.float32, device="cuda")
rstd = torch.empty(rows, dtype=torch.float32, device="cuda")
out = torch.empty_like(x)
_C.layer_norm_fwd(out, x, None, None, g, b, mean, rstd, 1e-5)
dx = torch.empty_like(x)
dgamma = torch.zeros(cols, dtype=torch.float32, device="cuda")
dbeta = torch.zeros(cols, dtype=torch.float32, device="cuda")

res = torch.randn_like(x)
s_out = torch.empty_like(x)


def timed(fn, nbytes, label, reps=5):
    """median and min of ``reps`` timings of 50 calls each"""
    for _ in range(10): fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(50): fn()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0)/50*1e6)
    us.sort()
    med = us[len(us)//2]
    print(f"{label} b128-shape: {med:.1f} us  {nbytes/med/1e6:.2f} TB/s"
          f"  (min {us[0]:.1f} us over {reps} x 50 calls)")


def run():
    _C.layer_norm_bwd(dx, dgamma, dbeta, dy, x, g, mean, rstd)
def fwd():
    _C.layer_norm_fwd(out, x, None, None, g, b, mean, rstd, 1e-5)
def fwd_res():
    _C.layer_norm_fwd(out, x, res, s_out, g, b, mean, rstd, 1e-5)
timed(fwd, rows*cols*2*2 + cols*4, "ln_fwd")
timed(fwd_res, rows*cols*2*4 + cols*4, "ln_fwd_res")
timed(run, rows*cols*2*3 + cols*2, "ln_bwd", reps=1)
