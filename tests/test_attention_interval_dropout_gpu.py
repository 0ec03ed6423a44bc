"""In-kernel dropout of the interval attention kernels
(csrc/kernels/attention_interval_drop.hip), through _C.attn_fwd_interval /
_C.attn_bwd_interval on guarded buffers.

* trivial bounds: the bits of the MHA dropout kernels (mask words, out,
  lse, dq, dk, dv) — the keying, the order of operations and the LDS mask
  staging against the global-load bodies, with no tolerance;
* real intervals: the fp64 reference of kernel_refs.py under the mask the
  forward published, |got - ref| <= ATTN_FACTOR x attn_bounds (dk / dv and
  their bounds summed over each group), exact zeros on padded rows, intact
  guards, and the keep rate of the visible elements;
* SelfAttention routes training-mode dropout to the native path, and a
  checkpointed recompute draws the same bits."""

import functools

import pytest
import torch

from tests import kernel_refs as kr
from tests.attn_group_cases import group_inputs
from tests.test_attention_band_cpu import doc_ids

pytestmark = pytest.mark.gpu

F64 = torch.float64
BF16 = torch.bfloat16
B = 2
# name -> (seq, lens): documents cut at a one-token document, inside a
# wave's 32 rows, on the block edge and into a tail block; a symmetric
# window; prefix-LM; a sample shorter than a block and an empty one
CASES = {"docs": (257, None), "win40": (200, None), "prefix33": (129, None),
         "docs_lens": (257, [100, 0])}
CUTS = (1, 33, 128, 200)


@functools.lru_cache(maxsize=None)
def mask_of(name):
    """[B, 1, S, S] bool by the definition (a padded row keeps its diagonal
    so that the reference stays finite); shared, nobody writes into it"""
    seq, lens = CASES[name]
    i, j = torch.arange(seq)[:, None], torch.arange(seq)[None, :]
    if name == "win40":
        valid = (i - j).abs() < 40
    elif name == "prefix33":
        valid = (j <= i) | (j < 33)
    else:
        ids = torch.cumsum(torch.bincount(torch.tensor(CUTS),
                                          minlength=seq), 0)
        valid = ids[:, None] == ids[None, :]
    valid = valid.expand(B, 1, seq, seq).clone()
    for n, ln in enumerate(lens or []):
        valid[n, 0, ln:] = False
        valid[n, 0, :, ln:] = False
    return valid | (i == j)


def bounds_of(name):
    from easyparallellibrary_amd.ops.attention import interval_bounds
    seq = CASES[name][0]
    if name == "win40":
        return interval_bounds(None, 40, seq, "cuda")
    if name == "prefix33":
        pos = torch.arange(seq, dtype=torch.int32, device="cuda")[None]
        return (torch.zeros_like(pos), pos.clamp(min=32) + 1,
                torch.where(pos < 33, 0, pos).int(),
                torch.full_like(pos, seq))
    ids = doc_ids(seq, CUTS)[None].expand(B, seq).cuda()
    return interval_bounds(ids, None, seq, "cuda")


def run(q, k, v, dout, bounds, lens, thresh, seed=1234, mha=False):
    """forward + backward on guarded buffers; results on the CPU, the mask
    as int32 [B, H, S, ceil(S / 32)].  mha: the dense dropout kernels"""
    from easyparallellibrary_amd import _C
    (b, h, seq, d), hkv = q.shape, k.shape[1]
    lq = kr.attn_layout("plain", b, h, seq, d, "cuda")
    lkv = kr.attn_layout("plain", b, hkv, seq, d, "cuda")
    lq["q"].copy_(q.to(BF16))
    lq["dout"].copy_(dout.to(BF16))
    lkv["k"].copy_(k.to(BF16))
    lkv["v"].copy_(v.to(BF16))
    lse, delta = (kr.attn_flat(b * h * seq, torch.float32, "cuda")
                  for _ in range(2))
    mask = kr.attn_flat(b * h * seq * ((seq + 31) // 32), torch.int32,
                        "cuda")
    sl = None if lens is None else torch.tensor(lens, dtype=torch.int32,
                                                device="cuda")
    scale, inv_keep = d ** -0.5, kr.attn_inv_keep(thresh)
    if mha:
        _C.attn_fwd(lq["q"], lkv["k"], lkv["v"], lq["out"], lse.view, scale,
                    False, mask.view, seed, thresh, inv_keep, sl)
        _C.attn_bwd(lq["q"], lkv["k"], lkv["v"], lq["out"], lq["dout"],
                    lse.view, delta.view, lq["dq"], lkv["dk"], lkv["dv"],
                    scale, False, True, mask.view, inv_keep, None, sl)
    else:
        _C.attn_fwd_interval(lq["q"], lkv["k"], lkv["v"], lq["out"],
                             lse.view, scale, *bounds[:2], sl, mask.view,
                             seed, thresh, inv_keep)
        _C.attn_bwd_interval(lq["q"], lkv["k"], lkv["v"], lq["out"],
                             lq["dout"], lse.view, delta.view, lq["dq"],
                             lkv["dk"], lkv["dv"], scale, *bounds, sl,
                             mask.view, inv_keep)
    torch.cuda.synchronize()
    guards = [lse, delta, mask, *lq["buffers"].values(),
              *lkv["buffers"].values()]
    assert sum(g.stray_writes() for g in guards) == 0
    got = dict(out=lq["out"].cpu(), dq=lq["dq"].cpu(), dk=lkv["dk"].cpu(),
               dv=lkv["dv"].cpu(), lse=lse.view.cpu().view(b, h, seq))
    return got, mask.view.cpu().view(b, h, seq, -1)


@pytest.mark.parametrize("lens", [None, "short"])
@pytest.mark.parametrize("thresh", [26, 128])
@pytest.mark.parametrize("seq", [72, 200, 257])
@pytest.mark.parametrize("d", [64, 128])
def test_trivial_bounds_give_the_mha_dropout_bits(d, seq, thresh, lens):
    lens = None if lens is None else [seq - 7, 40]
    inp = group_inputs("randn", seq, d, 3, 3, B)
    zero = torch.zeros(B, seq, dtype=torch.int32, device="cuda")
    bounds = (zero, zero + seq, zero, zero + seq)
    want, wmask = run(*inp, None, lens, thresh, mha=True)
    got, gmask = run(*inp, bounds, lens, thresh)
    again, amask = run(*inp, bounds, lens, thresh)
    _, other = run(*inp, bounds, lens, thresh, seed=99)
    for n in range(B):
        ln = seq if lens is None else lens[n]
        assert torch.equal(gmask[n, :, :ln], wmask[n, :, :ln])
        assert torch.equal(gmask[n, :, :ln], amask[n, :, :ln])
        assert not torch.equal(gmask[n, :, :ln], other[n, :, :ln])
    for name, t in got.items():
        bits = torch.int16 if t.dtype == BF16 else torch.int32
        assert torch.equal(t.view(bits), want[name].view(bits)), name
        assert torch.equal(t.view(bits), again[name].view(bits)), name


@pytest.mark.parametrize("thresh", [26, 128, 255])
@pytest.mark.parametrize("h,hkv", [(3, 3), (4, 1), (8, 2)])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("case", list(CASES))
def test_interval_dropout_against_fp64(case, d, h, hkv, thresh):
    (seq, lens), valid = CASES[case], mask_of(case)
    q, k, v, dout = group_inputs("randn", seq, d, h, hkv, B, valid, lens=lens)
    got, mask = run(q, k, v, dout, bounds_of(case), lens, thresh)
    keep = kr.unpack_keep(mask, B * h, seq).view(B, h, seq, seq)
    live = torch.zeros(B, 1, seq, 1, dtype=torch.bool)
    for n in range(B):
        live[n, 0, :seq if lens is None else lens[n]] = True
    # a word the forward did not write is the guard's sentinel: only bits
    # of visible elements count
    seen = (valid & live).expand_as(keep)
    rate = float(keep[seen].mean())
    print("INTERVAL-DROP keep rate {:.4f}".format(rate))
    assert abs(rate - (1 - thresh / 256)) <= 0.02, rate
    ke, ve = (t.repeat_interleave(h // hkv, dim=1) for t in (k, v))
    ref = kr.attn_ref(q, ke, ve, dout, False, d ** -0.5, keep=keep * seen,
                      inv_keep=kr.attn_inv_keep(thresh), valid=valid)
    limits = kr.attn_bounds(ref, q, ke, ve, dout, d ** -0.5)
    for name, t in got.items():
        want, bound = ref[name], limits[name]
        if name in ("dk", "dv"):
            want, bound = (x.view(B, hkv, h // hkv, seq, d).sum(2)
                           for x in (want, bound))
        t = t.to(F64)
        assert bool(torch.isfinite(t).all()), name
        for n in range(B):
            ln = seq if lens is None else lens[n]
            assert not bool(t[n, :, ln:].abs().any()), name
            ratio = kr.attn_ratio((t[n, :, :ln] - want[n, :, :ln]).abs(),
                                  bound[n, :, :ln]) if ln else 0.0
            print("INTERVAL-DROP-RATIO {} {:.3f}".format(name, ratio))
            assert ratio <= kr.ATTN_FACTOR[name], (name, n, ratio)


def test_selfattention_routes_interval_dropout_native():
    """training mode hands dropout to qkv_interval_attention, eval hands 0;
    a checkpointed forward + backward reproduces the gradients bitwise"""
    import torch.utils.checkpoint as cp
    import easyparallellibrary_amd.ops.attention as A
    from easyparallellibrary_amd.models.transformer import SelfAttention
    torch.manual_seed(3)
    m = SelfAttention(256, 4, dropout=0.1).to("cuda", BF16)
    x0 = torch.randn(B, 128, 256, device="cuda", dtype=BF16)
    ids = doc_ids(128, (1, 33, 100))[None].expand(B, 128).cuda()
    bounds = A.interval_bounds(ids, None, 128, "cuda")
    seen, orig = [], A.qkv_interval_attention

    def spy(qkv, bounds, scale=None, seqlens=None, dropout_p=0.0):
        seen.append(dropout_p)
        return orig(qkv, bounds, scale=scale, seqlens=seqlens,
                    dropout_p=dropout_p)

    def grads(fn):
        torch.manual_seed(5)
        x = x0.clone().requires_grad_()
        m.zero_grad()
        fn(x).float().sum().backward()
        return x.grad.clone(), m.qkv.weight.grad.clone()

    A.qkv_interval_attention = spy
    try:
        m.train()
        plain = grads(lambda x: m(x, bounds=bounds))
        ckpt = grads(lambda x: cp.checkpoint(
            lambda y: m(y, bounds=bounds), x, use_reentrant=False))
        m.eval()
        m(x0, bounds=bounds)
    finally:
        A.qkv_interval_attention = orig
    assert seen == [0.1, 0.1, 0.1, 0.0], seen
    for a, b in zip(plain, ckpt):
        assert bool(torch.isfinite(a.float()).all())
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
