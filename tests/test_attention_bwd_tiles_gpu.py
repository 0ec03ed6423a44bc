"""Attention backward tile bodies: transposed LDS reads, hardware bf16
convert, row constants from LDS (csrc/kernels/attention.hip).

* tr_read_probe: the ds_read_b64_tr_b16 fragments equal their 2-byte
  gather definition and the index-coded image, for both head dims.
* gradients: at the smallest shapes that reach every path, the max-abs
  error of dq/dk/dv against the fp32 torch reference with the new tiles
  is at most 1.25 x the error with EPL_ATTN_BWD_TILES=legacy on the
  same inputs plus one bf16 ulp of that gradient's max magnitude (the
  accumulator-initialised row constants and exp2 reorder one rounding;
  a lane-map or transposition mistake is an O(1) error).

EPL_ATTN_BWD_TILES and EPL_ATTN_BWD_DBUF are read once per process, so
each (tiles, dbuf) setting runs all cases in one fresh child process;
the four children run side by side, once per session.
"""

import json
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H = 2, 2
SEQS = (64,    # one chunk, waves 2 and 3 inactive
        72,    # 8-row tail: clamped rows under the transposed read
        200,   # tail inside the second 128-key block
        256)   # two blocks, bulk phase only
DROP_CASE = "d64-s200-full-plain-drop"


def case_ids():
    ids = ["d{}-s{}-{}-{}".format(d, s, "causal" if c else "full", layout)
           for d in (64, 128) for s in SEQS for c in (False, True)
           for layout in ("plain", "qkv")]
    return ids + [DROP_CASE]


def parse_case(cid):
    parts = cid.split("-")
    return dict(d=int(parts[0][1:]), seq=int(parts[1][1:]),
                causal=parts[2] == "causal", qkv=parts[3] == "qkv",
                drop=len(parts) > 4)


# --------------------------------------------------------------------------
# worker (child process): grads of every case vs the fp32 reference
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


def _unpack_keep(mask_words, bh, s):
    """keep bits [bh, s, s] from the forward's published mask words"""
    words = mask_words.reshape(bh, s, (s + 31) // 32)
    shifts = torch.arange(32, device=words.device)
    bits = ((words.unsqueeze(-1) >> shifts) & 1).reshape(bh, s, -1)
    return bits[:, :, :s].float()


def _worker(out_path):
    sys.path.insert(0, REPO)
    import easyparallellibrary_amd as epl
    from easyparallellibrary_amd.ops.attention import (
        _FlashAttention, flash_attention, qkv_flash_attention)
    epl.init()
    res = {}
    for idx, cid in enumerate(case_ids()):
        c = parse_case(cid)
        d, seq, causal = c["d"], c["seq"], c["causal"]
        scale = 1.0 / math.sqrt(d)
        torch.manual_seed(100 + idx)
        qkv = torch.randn(B, seq, 3, H, d).to("cuda", torch.bfloat16)
        dout = torch.randn(B, H, seq, d).to("cuda", torch.bfloat16)
        keep, inv_keep = None, 1.0
        if c["qkv"]:
            qkv.requires_grad_(True)
            out = qkv_flash_attention(qkv, causal=causal, scale=scale)
            out.backward(dout)
            q, k, v = (qkv.detach()[:, :, i].transpose(1, 2)
                       for i in range(3))
            got = [qkv.grad[:, :, i].transpose(1, 2) for i in range(3)]
        else:
            q, k, v = (qkv[:, :, i].transpose(1, 2).contiguous()
                       .requires_grad_(True) for i in range(3))
            if c["drop"]:
                out = _FlashAttention.apply(q, k, v, causal, scale, 0.5)
                saved = out.grad_fn.saved_tensors
                assert len(saved) == 6, "mask not saved"
                keep = _unpack_keep(saved[5], B * H, seq).reshape(
                    B, H, seq, seq)
                inv_keep = 256.0 / (256 - 128)
            else:
                out = flash_attention(q, k, v, causal=causal, scale=scale)
            out.backward(dout)
            got = [q.grad, k.grad, v.grad]
        assert "FlashAttention" in type(out.grad_fn).__name__, cid
        want = _ref_grads(q, k, v, dout, causal, scale, keep, inv_keep)
        torch.cuda.synchronize()
        res[cid] = {
            name: [(g.float() - w).abs().max().item(),
                   w.abs().max().item()]
            for name, g, w in zip(("dq", "dk", "dv"), got, want)}
    with open(out_path, "w") as f:
        json.dump(res, f)


# --------------------------------------------------------------------------
# tests
# --------------------------------------------------------------------------
SETTINGS = [(tiles, dbuf) for tiles in ("new", "legacy") for dbuf in (0, 2)]


@pytest.fixture(scope="session")
def tile_errors(tmp_path_factory):
    """{(tiles, dbuf): {case: {grad: [err, refmax]}}} — four children"""
    tmp = tmp_path_factory.mktemp("bwd_tiles")
    procs = []
    for tiles, dbuf in SETTINGS:
        env = dict(os.environ)
        env.pop("EPL_ATTN_BWD_TILES", None)
        if tiles == "legacy":
            env["EPL_ATTN_BWD_TILES"] = "legacy"
        env["EPL_ATTN_BWD_DBUF"] = str(dbuf)
        out = tmp / "{}_{}.json".format(tiles, dbuf)
        cmd = [sys.executable]
        if sys.flags.no_user_site:
            cmd.append("-s")
        cmd += [os.path.abspath(__file__), "--worker", str(out)]
        procs.append((tiles, dbuf, out, subprocess.Popen(
            cmd, env=env, cwd=REPO, stdout=subprocess.PIPE,
            stderr=subprocess.STDOUT, text=True)))
    res = {}
    for tiles, dbuf, out, p in procs:
        log, _ = p.communicate(timeout=600)
        assert p.returncode == 0, (tiles, dbuf, log[-3000:])
        with open(out) as f:
            res[(tiles, dbuf)] = json.load(f)
    return res


def bf16_ulp(x):
    """spacing of bf16 (8 significand bits) at magnitude x"""
    return 2.0 ** (math.floor(math.log2(x)) - 7) if x > 0 else 0.0


def _cases_x_dbuf():
    """d64 runs both staging modes; head_dim 128 always stages directly"""
    return [(cid, dbuf) for cid in case_ids()
            for dbuf in ((0, 2) if parse_case(cid)["d"] == 64 else (0,))]


@pytest.mark.parametrize("cid,dbuf", _cases_x_dbuf())
def test_new_tiles_match_legacy_error(tile_errors, cid, dbuf):
    new = tile_errors[("new", dbuf)][cid]
    old = tile_errors[("legacy", dbuf)][cid]
    for name in ("dq", "dk", "dv"):
        err_new, refmax = new[name]
        err_old, refmax_old = old[name]
        # same inputs, same fp32 reference in both children
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
