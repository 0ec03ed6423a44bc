"""Attention backward tile bodies: transposed LDS reads, hardware bf16
convert, row constants from LDS (csrc/kernels/attention.hip).

* tr_read_probe: the ds_read_b64_tr_b16 fragments equal their 2-byte
  gather definition and the index-coded image, for both head dims.
* gradients through the autograd entry points (flash_attention,
  qkv_flash_attention, _FlashAttention.apply with dropout) at the
  smallest shapes that reach every path, judged twice:
  - absolutely: dq, dk and dv on kernel_refs.attn_inputs("randn") against
    the fp64 reference of kernel_refs.py with its derived per-element
    bounds, err <= ATTN_FACTOR x E, and finite
    (test_kernel_refs_cpu.py proves the bounds at 1 x E on these cases
    and shows that they reject lane-map and transposition mistakes);
  - against the bodies these replaced (2-byte LDS gathers, software
    rounding, row constants from global memory): the max-abs error
    against the fp32 torch reference is at most 1.25 x theirs on the same
    inputs plus one bf16 ulp of that gradient's max magnitude.  Those
    bodies are deleted; their errors, recorded on an MI355X from the last
    build that had them, are tests/golden/attn_bwd_legacy_tile_errors.json
    ({dbuf: {case: {grad: [err, max|ref|]}}}).

EPL_ATTN_BWD_DBUF is read once per process, so each staging mode runs all
cases in one fresh child process; the two children run side by side, once
per session, and the parent judges their gradients against one fp64
reference per (d, seq, causal).
"""

import functools
import json
import math
import os
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, REPO)

from tests import kernel_refs as kr  # noqa: E402

pytestmark = pytest.mark.gpu

SEQS = kr.ATTN_AUTOGRAD_SEQS
DROP_D, DROP_SEQ, DROP_CAUSAL, DROP_THRESH = kr.ATTN_AUTOGRAD_DROP
DROP_CASE = "d{}-s{}-full-plain-drop".format(DROP_D, DROP_SEQ)
GRADS = ("dq", "dk", "dv")
DBUFS = (0, 2)
RECORDED = os.path.join(REPO, "tests", "golden",
                        "attn_bwd_legacy_tile_errors.json")
RECORDED_B, RECORDED_H = 2, 2     # the shape of the recording's inputs


def case_ids():
    ids = ["d{}-s{}-{}-{}".format(d, s, "causal" if c else "full", layout)
           for d in kr.ATTN_DIMS for s in SEQS for c in (False, True)
           for layout in ("plain", "qkv")]
    return ids + [DROP_CASE]


def parse_case(cid):
    parts = cid.split("-")
    return dict(d=int(parts[0][1:]), seq=int(parts[1][1:]),
                causal=parts[2] == "causal", qkv=parts[3] == "qkv",
                drop=len(parts) > 4)


# --------------------------------------------------------------------------
# worker (child process): every case on both input sets
# --------------------------------------------------------------------------
def _ref_grads(q, k, v, dout, causal, scale, keep=None, inv_keep=1.0):
    qf = q.detach().float().requires_grad_(True)
    kf = k.detach().float().requires_grad_(True)
    vf = v.detach().float().requires_grad_(True)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    if causal:
        n = q.shape[-2]
        s = s.masked_fill(torch.triu(torch.ones(
            n, n, device=q.device, dtype=torch.bool), 1), float("-inf"))
    p = s.softmax(dim=-1)
    if keep is not None:
        p = p * keep * inv_keep
    torch.matmul(p, vf).backward(dout.float())
    return qf.grad, kf.grad, vf.grad


def _kernel_grads(c, q, k, v, dout):
    """dq, dk, dv of one case through its entry point and the published
    mask words (dropout case) or None; q, k, v, dout: bf16 [B,H,seq,d]"""
    from easyparallellibrary_amd.ops.attention import (
        _FlashAttention, flash_attention, qkv_flash_attention)
    causal, scale, words = c["causal"], c["d"] ** -0.5, None
    if c["qkv"]:
        # [B, seq, 3, H, d]: the kernels consume the unbind views
        qkv = torch.stack([q, k, v], dim=0).permute(1, 3, 0, 2, 4)
        qkv = qkv.contiguous().requires_grad_(True)
        out = qkv_flash_attention(qkv, causal=causal, scale=scale)
        out.backward(dout)
        got = [qkv.grad[:, :, i].transpose(1, 2) for i in range(3)]
    else:
        q, k, v = (t.detach().contiguous().requires_grad_(True)
                   for t in (q, k, v))
        if c["drop"]:
            out = _FlashAttention.apply(q, k, v, causal, scale,
                                        DROP_THRESH / 256.0)
            saved = out.grad_fn.saved_tensors
            assert len(saved) == 6, "mask not saved"
            words = saved[5]
        else:
            out = flash_attention(q, k, v, causal=causal, scale=scale)
        out.backward(dout)
        got = [q.grad, k.grad, v.grad]
    assert "FlashAttention" in type(out.grad_fn).__name__, c
    torch.cuda.synchronize()
    return got, words


def _worker(out_prefix):
    import easyparallellibrary_amd as epl
    epl.init()
    grads, errors = {}, {}
    for idx, cid in enumerate(case_ids()):
        c = parse_case(cid)
        d, seq, causal = c["d"], c["seq"], c["causal"]
        # the fp64-judged inputs: the gradients go back as they are
        inp = [t.to("cuda", torch.bfloat16)
               for t in kr.attn_inputs("randn", seq, d, causal)]
        got, words = _kernel_grads(c, *inp)
        grads[cid] = {name: g.cpu().contiguous()
                      for name, g in zip(GRADS, got)}
        if words is not None:
            grads[cid]["words"] = words.cpu()
        # the recording's inputs: max-abs errors against fp32 torch
        torch.manual_seed(100 + idx)
        qkv = torch.randn(RECORDED_B, seq, 3, RECORDED_H, d).to(
            "cuda", torch.bfloat16)
        dout = torch.randn(RECORDED_B, RECORDED_H, seq, d).to(
            "cuda", torch.bfloat16)
        q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
        got, words = _kernel_grads(c, q, k, v, dout)
        keep, inv_keep = None, 1.0
        if words is not None:
            keep = kr.unpack_keep(words, RECORDED_B * RECORDED_H, seq).reshape(
                RECORDED_B, RECORDED_H, seq, seq).float()
            inv_keep = kr.attn_inv_keep(DROP_THRESH)
        want = _ref_grads(q, k, v, dout, causal, d ** -0.5, keep, inv_keep)
        errors[cid] = {
            name: [(g.float() - w).abs().max().item(), w.abs().max().item()]
            for name, g, w in zip(GRADS, got, want)}
    torch.save(grads, out_prefix + ".pt")
    with open(out_prefix + ".json", "w") as f:
        json.dump(errors, f)


# --------------------------------------------------------------------------
# tests
# --------------------------------------------------------------------------
@pytest.fixture(scope="session")
def children(tmp_path_factory):
    """{dbuf: (gradients {case: {dq, dk, dv[, words]}},
               errors {case: {grad: [err, refmax]}})} — two children"""
    tmp = tmp_path_factory.mktemp("bwd_tiles")
    procs = []
    for dbuf in DBUFS:
        env = dict(os.environ)
        env["EPL_ATTN_BWD_DBUF"] = str(dbuf)
        out = str(tmp / "dbuf{}".format(dbuf))
        cmd = [sys.executable]
        if sys.flags.no_user_site:
            cmd.append("-s")
        cmd += [os.path.abspath(__file__), "--worker", out]
        procs.append((dbuf, out, subprocess.Popen(
            cmd, env=env, cwd=REPO, stdout=subprocess.PIPE,
            stderr=subprocess.STDOUT, text=True)))
    res = {}
    for dbuf, out, p in procs:
        log, _ = p.communicate(timeout=600)
        assert p.returncode == 0, (dbuf, log[-3000:])
        with open(out + ".json") as f:
            res[dbuf] = (torch.load(out + ".pt"), json.load(f))
    return res


def _ref_and_bounds(d, seq, causal, keep=None, thresh=0):
    q, k, v, dout = kr.attn_inputs("randn", seq, d, causal)
    scale = d ** -0.5
    ref = kr.attn_ref(q, k, v, dout, causal, scale, keep,
                      kr.attn_inv_keep(thresh))
    return ref, kr.attn_bounds(ref, q, k, v, dout, scale)


# both layouts and both staging modes share the reference of a shape
_plain_ref = functools.lru_cache(maxsize=None)(_ref_and_bounds)


def _cases_x_dbuf():
    """d64 runs both staging modes; head_dim 128 always stages directly"""
    return [(cid, dbuf) for cid in case_ids()
            for dbuf in (DBUFS if parse_case(cid)["d"] == 64 else (0,))]


@pytest.mark.parametrize("cid,dbuf", _cases_x_dbuf())
def test_autograd_grads_inside_bounds(children, cid, dbuf):
    c = parse_case(cid)
    got = children[dbuf][0][cid]
    if c["drop"]:
        # the reference is fed the mask this child's forward published
        keep = kr.unpack_keep(got["words"], kr.ATTN_B * kr.ATTN_H,
                              c["seq"]).reshape(kr.ATTN_B, kr.ATTN_H,
                                                c["seq"], c["seq"])
        ref, bounds = _ref_and_bounds(c["d"], c["seq"], c["causal"], keep,
                                      DROP_THRESH)
    else:
        ref, bounds = _plain_ref(c["d"], c["seq"], c["causal"])
    ratios, bad = {}, []
    for name in GRADS:
        g = got[name].to(torch.float64)
        assert g.shape == ref[name].shape, (cid, name, g.shape)
        ratios[name] = kr.attn_ratio((g - ref[name]).abs(), bounds[name])
        if not bool(torch.isfinite(g).all()):
            bad.append("{} not finite".format(name))
        if not ratios[name] <= kr.ATTN_FACTOR[name]:
            bad.append("{} err/E {:.3f} > {}".format(
                name, ratios[name], kr.ATTN_FACTOR[name]))
    print("ATTN-RATIO autograd-dbuf{} {} {}".format(dbuf, cid, " ".join(
        "{}={:.3f}".format(name, ratios[name]) for name in GRADS)))
    assert not bad, (cid, dbuf, bad)


def bf16_ulp(x):
    """spacing of bf16 (8 significand bits) at magnitude x"""
    return 2.0 ** (math.floor(math.log2(x)) - 7) if x > 0 else 0.0


@pytest.fixture(scope="session")
def recorded_errors():
    with open(RECORDED) as f:
        return {int(dbuf): cases for dbuf, cases in json.load(f).items()}


@pytest.mark.parametrize("cid,dbuf", _cases_x_dbuf())
def test_new_tiles_match_legacy_error(children, recorded_errors, cid, dbuf):
    new = children[dbuf][1][cid]
    old = recorded_errors[dbuf][cid]
    for name in GRADS:
        err_new, refmax = new[name]
        err_old, refmax_old = old[name]
        # same inputs, same fp32 reference as in the recording
        assert math.isclose(refmax, refmax_old, rel_tol=1e-4)
        bound = 1.25 * err_old + bf16_ulp(refmax)
        print("{} dbuf{} {}: new {:.3e} legacy {:.3e} bound {:.3e} "
              "max|ref| {:.3e}".format(cid, dbuf, name, err_new, err_old,
                                       bound, refmax))
        assert math.isfinite(err_new) and err_new <= bound, (
            cid, dbuf, name, err_new, err_old, bound)


@pytest.mark.parametrize("d", [64, 128])
def test_tr_read_probe(d):
    from easyparallellibrary_amd import _C
    nfrag = 4 * (d // 32)
    gather = torch.full((nfrag, 64, 8), -1, device="cuda",
                        dtype=torch.int16)
    tr = torch.full((nfrag, 64, 8), -2, device="cuda", dtype=torch.int16)
    _C.tr_read_probe(gather, tr, d)
    torch.cuda.synchronize()
    # definition: element j of lane l of fragment (sub, qc, dj) is
    # image[sub + 16*qc + 8*(l>>5) + j][32*dj + (l&31)] = row*256 + col
    frag = torch.arange(nfrag).reshape(-1, 1, 1)
    lane = torch.arange(64).reshape(1, -1, 1)
    j = torch.arange(8).reshape(1, 1, -1)
    dj = frag % (d // 32)
    sq = frag // (d // 32)            # (sub/32)*2 + qc
    row = (sq // 2) * 32 + (sq % 2) * 16 + 8 * (lane // 32) + j
    col = 32 * dj + lane % 32
    want = (row * 256 + col).to(torch.int16)
    assert torch.equal(gather.cpu(), want)
    assert torch.equal(tr.cpu(), gather.cpu())


if __name__ == "__main__":
    assert sys.argv[1] == "--worker", sys.argv
    _worker(sys.argv[2])
