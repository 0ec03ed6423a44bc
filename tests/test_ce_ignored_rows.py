"""Cross-entropy on batches where most rows are ignored and the ignored
rows' logits are garbage (NaN, +inf, -inf), as the logits of padded
positions may be.

ce_backward_kernel writes a row of +0 for an ignored row without reading
its logits or statistics; ce_rowstats_kernel, with skip_ignored on (what
_VocabParallelCE passes), gives such a row max 0, sumexp 1, target logit 0
without reading it.  Checked: everything returned is finite, ignored rows
have zero loss and an exact +0 gradient row (sign bit clear), live rows
meet the bounds of test_cross_entropy_gpu.py against the fp64 reference,
and with skip_ignored off ce_rowstats still returns the reference's
statistics on ignored rows.

Sizes: 37 x 1001 fp32 and bf16 (scalar path), 37 x 1024 bf16 (vector
path), as one shard and as three; about 85 % of the rows ignored;
ignore_index -100 and 0.  The autograd path runs on the CPU as well.
"""

import pytest
import torch

from tests import kernel_refs as kr
from tests.test_cross_entropy_gpu import _dlogits_tol, _loss_tol

F64 = torch.float64
ROWS = 37
SIZES = [(1001, torch.float32), (1001, torch.bfloat16),
         (1024, torch.bfloat16)]


def split3(vocab):
    if vocab % 8 == 0:
        return [vocab // 2, vocab // 4, vocab // 4]     # 512 / 256 / 256
    return [400, 336, vocab - 736]


def case(vocab, widths, dtype, ignore_index, poison=True):
    """ce_case with 6 of 7 rows ignored; returns (logits with the ignored
    rows poisoned, clean logits for the reference, targets, dloss)"""
    clean, targets, dloss, _ = kr.ce_case(ROWS, widths, dtype, ignore_index)
    targets = targets.clone()
    rows = torch.arange(ROWS)
    targets[rows % 7 != 0] = ignore_index
    ignored = targets == ignore_index
    assert 0.8 <= float(ignored.double().mean()) < 1.0
    assert (~ignored).any()
    logits = clean.clone()
    if poison:
        idx = ignored.nonzero().squeeze(1)
        for i, r in enumerate(idx.tolist()):
            logits[r] = (float("nan"), float("inf"), float("-inf"))[i % 3]
        # one ignored row with a single bad element among finite ones
        logits[idx[-1]] = clean[idx[-1]]
        logits[idx[-1], vocab // 2] = float("nan")
    clean = clean.clone()
    clean[ignored] = 0          # the reference never looks at them
    return logits, clean, targets, dloss, ignored


def check_result(losses, dlogits, clean, targets, dloss, ignored,
                 ignore_index, dtype, scale=1.0):
    loss_ref, dlog_ref = kr.ce_ref(clean, targets, ignore_index, dloss, scale)
    losses = losses.detach().cpu().to(F64)
    got = dlogits.detach().cpu()
    assert torch.isfinite(losses).all() and torch.isfinite(got).all()
    assert (losses[ignored] == 0).all()
    assert (got[ignored] == 0).all()
    assert not torch.signbit(got[ignored]).any()
    live = ~ignored
    loss_err = (losses - loss_ref).abs()
    assert (loss_err <= _loss_tol(loss_ref, dtype)).all(), loss_err.max()
    dl = torch.where(live, dloss.to(F64) * scale,
                     torch.zeros(ROWS, dtype=F64))
    tol = _dlogits_tol(dlog_ref, dl, dtype)
    err = (got.to(F64) - dlog_ref).abs()
    assert (err <= tol).all(), (err / tol.clamp_min(1e-300))[live].max()


def kernel_path(vocab, dtype, ignore_index, shards):
    """the kernels per shard, merged as _VocabParallelCE.forward merges"""
    from easyparallellibrary_amd import _C
    widths = [vocab] if shards == 1 else split3(vocab)
    logits, clean, targets, dloss, ignored = case(vocab, widths, dtype,
                                                  ignore_index)
    dev = torch.device("cuda:0")
    tg = targets.to(dev)
    parts, stats, begins, b = [], [], [], 0
    for w in widths:
        sd = logits[:, b:b + w].contiguous().to(dev)
        lmax, lsum, tl = (torch.full((ROWS,), float("nan"), device=dev)
                          for _ in range(3))
        _C.ce_rowstats(sd, tg, lmax, lsum, tl, b, ignore_index,
                       skip_ignored=True)
        ig = ignored.to(dev)
        assert (lmax[ig] == 0).all() and (lsum[ig] == 1).all()
        assert (tl[ig] == 0).all()
        parts.append(sd)
        stats.append((lmax, lsum, tl))
        begins.append(b)
        b += w
    gmax = torch.stack([s[0] for s in stats]).max(dim=0).values
    gsum = torch.zeros_like(gmax)
    tlogit = torch.zeros_like(gmax)
    for lmax, lsum, tl in stats:
        gsum = gsum + lsum * torch.exp(lmax - gmax)
        tlogit = tlogit + tl
    assert (gsum[ignored.to(dev)] == len(widths)).all()
    losses = torch.where(tg != ignore_index,
                         torch.log(gsum) + gmax - tlogit,
                         torch.zeros_like(gmax))
    # garbage statistics on ignored rows must not matter either
    gmax_b = torch.where(ignored.to(dev), torch.full_like(gmax, float("nan")),
                         gmax)
    outs = []
    for sd, vb in zip(parts, begins):
        dlog = torch.full_like(sd, float("nan"))
        _C.ce_backward(dlog, sd, tg, gmax_b.contiguous(), gsum.contiguous(),
                       dloss.to(dev), vb, ignore_index, 0.5)
        outs.append(dlog)
    torch.cuda.synchronize()
    check_result(losses, torch.cat(outs, dim=1), clean, targets, dloss,
                 ignored, ignore_index, dtype, scale=0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("shards", [1, 3])
@pytest.mark.parametrize("ignore_index", [-100, 0])
@pytest.mark.parametrize("vocab,dtype", SIZES)
def test_ce_kernels_skip_ignored_rows(vocab, dtype, ignore_index, shards):
    kernel_path(vocab, dtype, ignore_index, shards)


@pytest.mark.gpu
@pytest.mark.parametrize("ignore_index", [-100, 0])
@pytest.mark.parametrize("vocab,dtype", SIZES)
def test_ce_rowstats_default_reads_ignored_rows(vocab, dtype, ignore_index):
    """skip_ignored off (the default): today's values on ignored rows"""
    from easyparallellibrary_amd import _C
    widths = split3(vocab)
    logits, _, targets, _, ignored = case(vocab, widths, dtype, ignore_index,
                                          poison=False)
    dev = torch.device("cuda:0")
    b = 0
    for w in widths:
        shard = logits[:, b:b + w].contiguous()
        lmax, lsum, tl = (torch.full((ROWS,), float("nan"), device=dev)
                          for _ in range(3))
        _C.ce_rowstats(shard.to(dev), targets.to(dev), lmax, lsum, tl, b,
                       ignore_index)
        rmax, rsum, rtl = kr.ce_shard_stats_ref(shard, targets, b,
                                                ignore_index)
        assert torch.equal(lmax.cpu().to(F64), rmax)
        assert torch.equal(tl.cpu().to(F64), rtl)
        rel = (lsum.cpu().to(F64) - rsum).abs() / rsum
        assert (rel <= (1e-5 if dtype == torch.bfloat16 else 1e-4)).all()
        assert ignored.any()
        b += w


def autograd_path(device, vocab, dtype, ignore_index):
    from easyparallellibrary_amd.ops.distributed_losses import (
        vocab_parallel_cross_entropy)
    logits, clean, targets, dloss, ignored = case(vocab, [vocab], dtype,
                                                  ignore_index)
    lg = logits.to(device).requires_grad_(True)
    losses = vocab_parallel_cross_entropy(lg, targets.to(device),
                                          ignore_index=ignore_index)
    (losses * dloss.to(device)).sum().backward()
    check_result(losses, lg.grad, clean, targets, dloss, ignored,
                 ignore_index, dtype)


@pytest.mark.parametrize("ignore_index", [-100, 0])
@pytest.mark.parametrize("vocab,dtype", SIZES)
def test_ce_autograd_ignored_rows_cpu(vocab, dtype, ignore_index):
    autograd_path("cpu", vocab, dtype, ignore_index)


@pytest.mark.gpu
@pytest.mark.parametrize("ignore_index", [-100, 0])
@pytest.mark.parametrize("vocab,dtype", SIZES)
def test_ce_autograd_ignored_rows_gpu(vocab, dtype, ignore_index):
    import easyparallellibrary_amd as epl
    epl.init()
    autograd_path("cuda:0", vocab, dtype, ignore_index)
