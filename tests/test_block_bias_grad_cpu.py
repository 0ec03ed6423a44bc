"""Block with the LN-backward fusion switch on vs off, on the CPU in fp32.

With the switch on, the bias gradients of attn.proj and mlp.fc2 come out
of the following LayerNorm's backward and the summed stream's gradient is
added inside it.  That is the same mathematics in another order, so loss,
input gradient and every parameter gradient must agree to fp32 round-off
(atol = rtol = 1e-5).
"""

import pytest
import torch

from easyparallellibrary_amd.models.transformer import Block, init_weights
from easyparallellibrary_amd.ops import layer_norm
from easyparallellibrary_amd.ops.layer_norm import FusedLayerNorm

H, HEADS, B, S = 64, 2, 2, 16

# names and registration order of the parent's Block
PARAM_NAMES = [
    "ln1.weight", "ln1.bias",
    "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
    "ln2.weight", "ln2.bias",
    "mlp.fc1.weight", "mlp.act.bias", "mlp.fc2.weight", "mlp.fc2.bias",
]


def _make(pre_ln):
    torch.manual_seed(3)
    blk = init_weights(Block(H, HEADS, 4 * H, causal=pre_ln, pre_ln=pre_ln))
    with torch.no_grad():
        for n, p in blk.named_parameters():
            if n.endswith("bias"):
                p.normal_(std=0.1)
    x = torch.randn(B, S, H)
    w = torch.randn(B, S, H)
    return blk, x, w


def _run(blk, x, w):
    blk.zero_grad(set_to_none=True)
    xi = x.clone().requires_grad_(True)
    loss = (blk(xi) * w).sum()
    loss.backward()
    grads = {n: (None if p.grad is None else p.grad.clone())
             for n, p in blk.named_parameters()}
    return loss.detach(), xi.grad.clone(), grads


def _close(a, b):
    return torch.allclose(a, b, atol=1e-5, rtol=1e-5)


def _ab(blk, x, w, monkeypatch):
    monkeypatch.setattr(layer_norm, "_LN_BWD_FUSE", False)
    off = _run(blk, x, w)
    monkeypatch.setattr(layer_norm, "_LN_BWD_FUSE", True)
    on = _run(blk, x, w)
    return off, on


@pytest.mark.parametrize("pre_ln", [False, True])
def test_param_names_and_order(pre_ln):
    blk, _, _ = _make(pre_ln)
    assert [n for n, _ in blk.named_parameters()] == PARAM_NAMES
    assert list(blk.state_dict().keys()) == PARAM_NAMES


@pytest.mark.parametrize("pre_ln", [False, True])
def test_fused_matches_unfused(pre_ln, monkeypatch):
    blk, x, w = _make(pre_ln)
    (l0, dx0, g0), (l1, dx1, g1) = _ab(blk, x, w, monkeypatch)
    assert _close(l0, l1)
    assert _close(dx0, dx1)
    assert list(g1) == PARAM_NAMES
    for n in PARAM_NAMES:
        assert g0[n] is not None and g1[n] is not None, n
        assert _close(g0[n], g1[n]), n


@pytest.mark.parametrize("pre_ln", [False, True])
def test_fused_route_is_taken(pre_ln, monkeypatch):
    """The switch really moves the bias gradient: with it on, the LN node
    receives the Linear's bias as an input that needs a gradient."""
    blk, x, w = _make(pre_ln)
    seen = []
    orig = layer_norm._FusedLayerNorm.apply

    def spy(*args):
        seen.append(args[5] if len(args) > 5 else None)
        return orig(*args)

    monkeypatch.setattr(layer_norm._FusedLayerNorm, "apply", spy)
    monkeypatch.setattr(layer_norm, "_LN_BWD_FUSE", True)
    blk(x)
    want = ([None, blk.attn.proj.bias] if pre_ln
            else [blk.attn.proj.bias, blk.mlp.fc2.bias])
    assert len(seen) == 2 and all(a is b for a, b in zip(seen, want))
    seen.clear()
    monkeypatch.setattr(layer_norm, "_LN_BWD_FUSE", False)
    blk(x)
    assert seen == [None, None]


@pytest.mark.parametrize("pre_ln", [False, True])
def test_frozen_proj_bias_takes_unfused_route(pre_ln, monkeypatch):
    blk, x, w = _make(pre_ln)
    blk.attn.proj.bias.requires_grad_(False)
    seen = []
    orig = layer_norm._FusedLayerNorm.apply

    def spy(*args):
        seen.append(args[5] if len(args) > 5 else None)
        return orig(*args)

    monkeypatch.setattr(layer_norm._FusedLayerNorm, "apply", spy)
    (l0, dx0, g0), (l1, dx1, g1) = _ab(blk, x, w, monkeypatch)
    # the last forward ran with the switch on: proj's bias never reached
    # an LN node
    assert all(a is not blk.attn.proj.bias for a in seen)
    assert g0["attn.proj.bias"] is None and g1["attn.proj.bias"] is None
    assert _close(l0, l1) and _close(dx0, dx1)
    for n in PARAM_NAMES:
        if n != "attn.proj.bias":
            assert _close(g0[n], g1[n]), n


def test_forward_with_sum_only_y_used(monkeypatch):
    """Only y of forward_with_sum feeds the loss: ds is None in backward
    (no zero tensor is materialised) and the gradients are those of
    LN(a + r) alone — checked against torch's LayerNorm."""
    torch.manual_seed(4)
    ln = FusedLayerNorm(H)
    lin = torch.nn.Linear(H, H)
    with torch.no_grad():
        ln.weight.normal_()
        ln.bias.normal_()
    h = torch.randn(B * S, H)
    r = torch.randn(B * S, H)
    w = torch.randn(B * S, H)

    def ref():
        hi = h.clone().requires_grad_(True)
        ri = r.clone().requires_grad_(True)
        for p in list(ln.parameters()) + list(lin.parameters()):
            p.grad = None
        y = torch.nn.functional.layer_norm(lin(hi) + ri, (H,), ln.weight,
                                           ln.bias, ln.eps)
        (y * w).sum().backward()
        return [hi.grad, ri.grad, ln.weight.grad, ln.bias.grad,
                lin.weight.grad, lin.bias.grad]

    def fused():
        hi = h.clone().requires_grad_(True)
        ri = r.clone().requires_grad_(True)
        for p in list(ln.parameters()) + list(lin.parameters()):
            p.grad = None
        a, lb = layer_norm.linear_for_ln(lin, hi)
        y, _ = ln.forward_with_sum(a, ri, lin_bias=lb)
        (y * w).sum().backward()
        return [hi.grad, ri.grad, ln.weight.grad, ln.bias.grad,
                lin.weight.grad, lin.bias.grad]

    want = [g.clone() for g in ref()]
    for switch in (True, False):
        monkeypatch.setattr(layer_norm, "_LN_BWD_FUSE", switch)
        got = fused()
        for a, b in zip(got, want):
            assert a is not None and torch.allclose(a, b, atol=1e-5,
                                                    rtol=1e-5)


def test_forward_with_sum_only_s_used(monkeypatch):
    """Only the summed stream is used: dy is None, LN contributes nothing
    and the Linear's bias still gets its column sum."""
    torch.manual_seed(6)
    ln = FusedLayerNorm(H)
    lin = torch.nn.Linear(H, H)
    h = torch.randn(B * S, H)
    r = torch.randn(B * S, H, requires_grad=True)
    w = torch.randn(B * S, H)
    monkeypatch.setattr(layer_norm, "_LN_BWD_FUSE", True)
    a, lb = layer_norm.linear_for_ln(lin, h)
    assert lb is lin.bias
    _, s = ln.forward_with_sum(a, r, lin_bias=lb)
    (s * w).sum().backward()
    assert torch.allclose(r.grad, w)
    assert torch.allclose(lin.bias.grad, w.sum(0), atol=1e-5, rtol=1e-5)
    assert torch.allclose(lin.weight.grad, w.t() @ h, atol=1e-5, rtol=1e-5)
    assert ln.weight.grad is None and ln.bias.grad is None
