"""ce_rowstats / ce_backward called per vocabulary shard with its
vocab_begin, merged as _VocabParallelCE.forward merges them, against the
full-vocabulary fp64 reference (log_softmax, softmax - onehot) of
tests/kernel_refs.py on the same values.

Inputs are constructed (kernel_refs.ce_case): targets on both sides of
every shard edge, on the last column and on class 0; every 7th row
ignored; a row of logits around +100; rows whose peak is 60 and 120
above everything in the other shards (the far shards' rescaled sum is
negligible, respectively exactly 0 in fp32); a row of equal logits; all
other logits within +/-8.

Bounds.  row_max and target_logit are copies of inputs: exact.
row_sumexp: 256 partial sums of at most cols/256 terms, a 10-step tree
and expf at about 1 ulp bound the error near 2e-6; checked at rtol 1e-5
for bf16 inputs and at the project's fp32 tolerance 1e-4 for fp32 inputs
(there v - max is itself rounded, |v - max| * 2**-24 in the exponent).
Loss: 1e-5 + 1e-6 |loss| for bf16 inputs, 1e-4 relative for fp32 inputs
(the smallest live loss of any case is 0.29, so a relative bound is
meaningful everywhere).  dlogits: one bf16 ulp plus the exp error,
2**-8 |ref| + 1e-6 |dloss * scale|, for bf16; rtol 1e-4, atol
1e-7 |dloss * scale| for fp32.
"""

import pytest
import torch

from tests import kernel_refs as kr

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from easyparallellibrary_amd import _C
else:
    _C = None

F64 = torch.float64
SCALE = 0.5

CASES = [
    (5, [8], -100),                    # one shard, one vector
    (5, [7], -100),                    # scalar path, cols < threads
    (37, [2048, 2056, 1001], -100),    # one pass / one pass + 1 / scalar
    (37, [2048, 2056, 1001], 0),       # a legal class id as ignore value
    (1, [264, 264], -100),             # single row
    (4097, [264, 256], -100),          # one row past the 4096-block grid
]


def dev():
    return torch.device("cuda:0")


def _cpu64(t):
    return t.detach().cpu().to(F64)


def _loss_tol(ref, dtype):
    if dtype == torch.bfloat16:
        return 1e-5 + 1e-6 * ref.abs()
    return 1e-4 * ref.abs()


def _dlogits_tol(ref, dl, dtype):
    if dtype == torch.bfloat16:
        return 2.0 ** -8 * ref.abs() + 1e-6 * dl.abs()[:, None]
    return 1e-4 * ref.abs() + 1e-7 * dl.abs()[:, None]


@pytest.mark.parametrize("rows,widths,ignore_index", CASES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_ce_sharded(dtype, rows, widths, ignore_index):
    logits, targets, dloss, special = kr.ce_case(rows, widths, dtype,
                                                 ignore_index)
    vocab = sum(widths)
    ignored = targets == ignore_index
    live = ~ignored
    # the kernels index a row with target - vocab_begin when it lies in
    # the shard: every live target is a column of the full vocabulary
    assert int(targets[live].min()) >= 0 and int(targets[live].max()) < vocab
    if rows >= 7:
        assert ignored.any()
        for t in kr.ce_required_targets(widths):
            assert (targets == t).any()
    if ignore_index == 0:
        assert ignored.sum() > len(range(6, rows, 7))
    loss_ref, dlog_ref = kr.ce_ref(logits, targets, ignore_index, dloss,
                                   SCALE)

    tg = targets.to(dev())
    shards, stats, begins = [], [], []
    b = 0
    sum_rtol = 1e-5 if dtype == torch.bfloat16 else 1e-4
    worst_sum = 0.0
    for w in widths:
        shard = logits[:, b:b + w].contiguous()
        sd = shard.to(dev())
        assert sd.is_contiguous() and sd.shape == (rows, w)
        lmax, lsum, tl = (torch.full((rows,), float("nan"), device=dev())
                          for _ in range(3))
        _C.ce_rowstats(sd, tg, lmax, lsum, tl, b, ignore_index)
        torch.cuda.synchronize()
        rmax, rsum, rtl = kr.ce_shard_stats_ref(shard, targets, b,
                                                ignore_index)
        assert torch.equal(_cpu64(lmax), rmax)
        assert torch.equal(_cpu64(tl), rtl)
        outside = ignored | (targets < b) | (targets >= b + w)
        assert (_cpu64(tl)[outside] == 0).all()
        rel = ((_cpu64(lsum) - rsum).abs() / rsum)
        worst_sum = max(worst_sum, rel.max().item())
        assert (rel <= sum_rtol).all(), (b, rel.max())
        shards.append(sd)
        stats.append((lmax, lsum, tl))
        begins.append(b)
        b += w

    # _VocabParallelCE.forward's merge, in fp32 on the device
    gmax = torch.stack([s[0] for s in stats]).max(dim=0).values
    gsum = torch.zeros_like(gmax)
    tlogit = torch.zeros_like(gmax)
    for lmax, lsum, tl in stats:
        gsum = gsum + lsum * torch.exp(lmax - gmax)
        tlogit = tlogit + tl
    losses = torch.where(tg != ignore_index,
                         torch.log(gsum) + gmax - tlogit,
                         torch.zeros_like(gmax))
    if "gap120" in special:
        r = special["gap120"]
        far = stats[-1]
        assert (far[1] * torch.exp(far[0] - gmax))[r] == 0
    loss_err = (_cpu64(losses) - loss_ref).abs()
    loss_tol = _loss_tol(loss_ref, dtype)
    assert torch.isfinite(losses).all()
    assert (_cpu64(losses)[ignored] == 0).all()

    dl_dev = dloss.to(dev())
    parts = []
    for sd, vb in zip(shards, begins):
        dlog = torch.full_like(sd, float("nan"))
        _C.ce_backward(dlog, sd, tg, gmax.contiguous(), gsum.contiguous(),
                       dl_dev, vb, ignore_index, SCALE)
        parts.append(dlog)
    torch.cuda.synchronize()
    got = _cpu64(torch.cat(parts, dim=1))
    dl = torch.where(live, dloss.to(F64) * SCALE, torch.zeros(rows, dtype=F64))
    tol = _dlogits_tol(dlog_ref, dl, dtype)
    err = (got - dlog_ref).abs()
    tol_pos = tol.clamp_min(1e-300)
    print("%s rows %d widths %s ignore %d: max rel err sumexp %.3g (tol %g),"
          " max loss err %.3g (err/tol %.3g), max dlogits err %.3g "
          "(err/tol %.3g)"
          % (str(dtype).split(".")[-1], rows, widths, ignore_index, worst_sum,
             sum_rtol, loss_err.max().item(),
             (loss_err / loss_tol.clamp_min(1e-300)).max().item(),
             err.max().item(),
             (err / tol_pos)[live].max().item() if live.any() else 0.0))
    assert (loss_err <= loss_tol).all(), \
        (loss_err / loss_tol.clamp_min(1e-300)).max()
    assert torch.isfinite(got).all()
    assert (got[ignored] == 0).all()
    assert (err <= tol).all(), (err / tol_pos)[live].max()
    # the -1 sits on the target column exactly once per row
    row_sum = got.sum(dim=1).abs()
    assert (row_sum <= tol.sum(dim=1) + 1e-12).all()
    assert (got[live, targets[live]] <= 0).all()
    rest = got[live].clone()
    rest[torch.arange(int(live.sum())), targets[live]] = 0
    assert (rest >= 0).all()


def test_vocab_parallel_ce_function_fp32():
    """The autograd path on fp32 logits (37 x 1001, the scalar kernels)
    against torch.nn.functional.cross_entropy in fp64, at the fp32 bounds
    of test_ce_sharded."""
    import easyparallellibrary_amd as epl
    from easyparallellibrary_amd.ops.distributed_losses import (
        vocab_parallel_cross_entropy)
    epl.init()
    rows, vocab = 37, 1001
    logits, targets, dloss, _ = kr.ce_case(rows, [vocab], torch.float32)
    lg = logits.to(dev()).requires_grad_(True)
    losses = vocab_parallel_cross_entropy(lg, targets.to(dev()))
    (losses * dloss.to(dev())).sum().backward()
    torch.cuda.synchronize()

    lr = logits.to(F64).requires_grad_(True)
    want = torch.nn.functional.cross_entropy(lr, targets, ignore_index=-100,
                                             reduction="none")
    (want * dloss.to(F64)).sum().backward()
    ignored = targets == -100
    assert ignored.any()
    loss_err = (_cpu64(losses) - want.detach()).abs()
    assert (loss_err <= _loss_tol(want.detach(), torch.float32)).all()
    assert (_cpu64(losses)[ignored] == 0).all()
    dl = torch.where(ignored, torch.zeros(rows, dtype=F64), dloss.to(F64))
    tol = _dlogits_tol(lr.grad, dl, torch.float32)
    err = (_cpu64(lg.grad) - lr.grad).abs()
    print("fp32 autograd path: max loss err %.3g, max dlogits err %.3g "
          "(err/tol %.3g)" % (loss_err.max().item(), err.max().item(),
                              (err / tol.clamp_min(1e-300))[~ignored]
                              .max().item()))
    assert (err <= tol).all()
    assert (_cpu64(lg.grad)[ignored] == 0).all()
