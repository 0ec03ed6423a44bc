"""Mixture-of-Experts with expert parallelism (all-to-all dispatch/combine).

Capability parity: /root/reference/epl/parallel/hooks.py:758-794 (einsum
hook inserting all-to-all before the first and after the third einsum
around the expert weights) + parallel/ops.py:485-495 (alltoall with
optional fp16 compression) + csrc nccl_all_to_all.cc.

MI355X redesign: an explicit MoE layer — top-1/top-2 gating with capacity,
dispatch as ONE equal-split all-to-all over xGMI, local expert FFN batched
as a single bmm over the rank's experts, combine with the reverse
all-to-all.  The a2a autograd pair (a2a <-> a2a) lives in
comm/functional.py.

Router semantics (aux_loss_coef / z_loss_coef / fused_router; the torch
path ``router_torch`` and the kernels of csrc/kernels/moe_router.hip both
implement exactly this).  For logits z[N, E] (bf16 or fp32), in fp32:

- Softmax: m_t = max_e z_te, lse_t = m_t + log sum_e exp(z_te - m_t),
  p_te = exp(z_te - lse_t).
- Selection: the k largest z_te of the row, ties to the lower expert
  index.  The comparison is on the logits' values: exact, no rounding.
- Weights: w_tj = p_{t,i_j} / sum_l p_{t,i_l}; identically 1 with zero
  gradient for k = 1.
- Counts: c_e = number of (t, j) with topi[t, j] = e, before the capacity
  drop (int64; the tensor the slot assignment needs anyway).
- Losses: L_bal = E sum_e f_e P_e with f_e = c_e / (N k) (a constant in
  the backward) and P_e = (1/N) sum_t p_te; it is 1 at a uniform router.
  L_z = (1/N) sum_t lse_t^2.  The statistics are those of the call (this
  rank, this micro-batch); the router runs no collective.
- Backward, from dw[N, k] and the 0-dim fp32 device tensors g_bal, g_z:
  a_te = g_bal E f_e / N, plus (dw_tj - sum_l dw_tl w_tl) / S_t at the
  selected experts (S_t = sum_l p_{t,i_l}; nothing for k = 1), and
  dz_te = p_te (a_te - sum_e' p_te' a_te') + g_z (2 lse_t / N) p_te,
  rounded once to the logits' dtype.

The losses enter autograd where they arise (``_AttachAuxLoss``): the
layer's output carries them, so they reach the gate weights from any
pipeline stage, under gradient checkpointing and in a captured step.
"""

import torch
import torch.nn as nn
import torch.nn.functional as F

from easyparallellibrary_amd.comm import functional
from easyparallellibrary_amd.ops.dispatch import native_ext, use_native


def _moe_bmm():
    import os
    return os.environ.get("EPL_MOE_BMM", "1") == "1"


def _moe_native_dispatch():
    import os
    return os.environ.get("EPL_MOE_NATIVE_DISPATCH", "1") == "1"


def _moe_fused_router_env():
    import os
    return os.environ.get("EPL_MOE_FUSED_ROUTER")


# experts the router kernels take (csrc/kernels/moe_router.hip)
ROUTER_MIN_EXPERTS, ROUTER_MAX_EXPERTS = 2, 256

# Multiplier of the gradient _AttachAuxLoss hands its loss: the engine
# sets it to the AMP loss scale at the start of every step, so the aux
# gradients are scaled (and later unscaled) like the task loss's.
_aux_loss_scale = 1.0


def set_aux_loss_scale(scale):
    global _aux_loss_scale
    _aux_loss_scale = float(scale)


def get_aux_loss_scale():
    return _aux_loss_scale


def router_torch(logits, k):
    """The router semantics of the module docstring in torch ops (with
    autograd).  Returns topi [N, k] int64, topw [N, k] fp32, counts [E]
    int64, L_bal, L_z (0-dim fp32)."""
    z = logits.float()
    n, e = z.shape
    lse = torch.logsumexp(z, dim=-1)
    p = torch.exp(z - lse.unsqueeze(-1))
    # stable descending sort: equal logits keep the lower index first
    topi = torch.sort(z.detach(), dim=-1, descending=True,
                      stable=True).indices[:, :k].contiguous()
    if k == 1:
        topw = torch.ones(n, 1, dtype=torch.float32, device=z.device)
    else:
        topv = p.gather(1, topi)
        topw = topv / topv.sum(dim=-1, keepdim=True)
    counts = torch.zeros(e, dtype=torch.long, device=z.device)
    counts.scatter_add_(0, topi.reshape(-1),
                        torch.ones(n * k, dtype=torch.long, device=z.device))
    f = counts.to(torch.float32) / float(n * k)
    l_bal = float(e) * (f * p.mean(dim=0)).sum()
    l_z = (lse * lse).mean()
    return topi, topw, counts, l_bal, l_z


class _FusedRouter(torch.autograd.Function):
    """Router forward and backward as one kernel each
    (csrc/kernels/moe_router.hip) plus the small fold of the forward's
    partial rows.  Returns topi, topw, counts, L_bal, L_z."""

    @staticmethod
    def forward(ctx, logits, k):
        logits = logits.contiguous()
        n, e = logits.shape
        dev = logits.device
        topi = torch.empty(n, k, dtype=torch.long, device=dev)
        topw = torch.empty(n, k, dtype=torch.float32, device=dev)
        lse = torch.empty(n, dtype=torch.float32, device=dev)
        counts = torch.empty(e, dtype=torch.long, device=dev)
        psum = torch.empty(e, dtype=torch.float32, device=dev)
        losses = torch.empty(2, dtype=torch.float32, device=dev)
        native_ext().moe_router_fwd(logits, k, topi, topw, lse, counts,
                                    psum, losses)
        ctx.save_for_backward(logits, lse, topi, counts)
        ctx.k = k
        ctx.mark_non_differentiable(topi, counts)
        return topi, topw, counts, losses[0], losses[1]

    @staticmethod
    def backward(ctx, _dtopi, dw, _dcounts, g_bal, g_z):
        logits, lse, topi, counts = ctx.saved_tensors
        n = logits.shape[0]
        zero = None
        if dw is None or g_bal is None or g_z is None:
            zero = torch.zeros((), dtype=torch.float32,
                               device=logits.device)
        dw = (torch.zeros(n, ctx.k, dtype=torch.float32,
                          device=logits.device) if dw is None
              else dw.float().contiguous())
        g_bal = zero if g_bal is None else g_bal.float().contiguous()
        g_z = zero if g_z is None else g_z.float().contiguous()
        dlogits = torch.empty_like(logits)
        native_ext().moe_router_bwd(dlogits, logits, lse, topi, dw, counts,
                                    g_bal, g_z, ctx.k)
        return dlogits, None


class _AttachAuxLoss(torch.autograd.Function):
    """(out, aux) -> out.  Identity on ``out``; the backward passes dout
    through and gives the 0-dim loss ``aux`` the gradient coef * scale
    (``set_aux_loss_scale``), as if coef * aux had been added to the loss
    the step differentiates.  Division by the micro-batch count and the
    data-parallel average then apply to it as to the task loss."""

    @staticmethod
    def forward(ctx, out, aux, coef):
        ctx.coef = float(coef)
        ctx.aux_shape = aux.shape
        ctx.aux_dtype = aux.dtype
        return out.view_as(out)

    @staticmethod
    def backward(ctx, dout):
        g = torch.full(ctx.aux_shape, ctx.coef * _aux_loss_scale,
                       dtype=ctx.aux_dtype, device=dout.device)
        return dout, g, None


def moe_aux_losses(model):
    """Sums over the model's ExpertParallelMLP layers of the detached
    losses of their last forward: dict(balance_loss=, z_loss=) of 0-dim
    tensors, or None values when no layer has computed them."""
    bal, zl = None, None
    for m in model.modules():
        if isinstance(m, ExpertParallelMLP) and \
                m.last_balance_loss is not None:
            bal = m.last_balance_loss if bal is None \
                else bal + m.last_balance_loss
            zl = m.last_z_loss if zl is None else zl + m.last_z_loss
    return dict(balance_loss=bal, z_loss=zl)


class _MoEDispatch(torch.autograd.Function):
    """Fused token dispatch (csrc/kernels/moe.hip): one wave copies one
    hidden row per kept assignment; over-capacity entries are skipped
    INLINE (no boolean compaction, no nonzero device->host sync).
    Backward gathers each token's k slot-gradients (dropped -> zero)."""

    @staticmethod
    def forward(ctx, x, fe, pos, ft, inv, k, capacity, num_experts):
        disp = x.new_zeros(num_experts, capacity, x.shape[-1])
        native_ext().moe_dispatch_fwd(disp, x, fe, pos, ft, capacity)
        ctx.save_for_backward(fe, pos, inv)
        ctx.k = k
        ctx.cap = capacity
        ctx.n = x.shape[0]
        return disp

    @staticmethod
    def backward(ctx, ddisp):
        fe, pos, inv = ctx.saved_tensors
        dx = ddisp.new_empty(ctx.n, ddisp.shape[-1])
        native_ext().moe_dispatch_bwd(dx, ddisp.contiguous(), fe, pos,
                                      inv, ctx.k, ctx.cap)
        return dx, None, None, None, None, None, None, None


class _MoECombine(torch.autograd.Function):
    """Fused weighted combine: out[t] = sum_j fw * h[slot_j(t)] with
    fp32 accumulation; backward writes dh rows (unique slots, no
    atomics) and per-assignment dfw dot products."""

    @staticmethod
    def forward(ctx, h, fw, fe, pos, ft, inv, k, capacity, n_tokens):
        h = h.contiguous()
        fwf = fw.detach().float().contiguous()
        out = h.new_empty(n_tokens, h.shape[-1])
        native_ext().moe_combine_fwd(out, h, fwf, fe, pos, inv, k,
                                     capacity)
        ctx.save_for_backward(h, fwf, fe, pos, ft)
        ctx.cap = capacity
        return out

    @staticmethod
    def backward(ctx, dout):
        h, fwf, fe, pos, ft = ctx.saved_tensors
        dh = torch.zeros_like(h)
        dfw = torch.empty_like(fwf)
        native_ext().moe_combine_bwd(dh, dfw, dout.contiguous(), h, fwf,
                                     fe, pos, ft, ctx.cap)
        return dh, dfw, None, None, None, None, None, None, None


class _BatchedExpertLinear(torch.autograd.Function):
    """Per-expert batched GEMM with a hand-written backward.

    torch.bmm's own autograd backward memory-faults on
    ROCm 7.0.x/gfx950 (still reproduced on 7.0.2 —
    gpurun_out/r2_moe_bmm2.txt, repro tests/moe_bisect_gpu.py bmm2).
    Issuing the backward GEMMs OURSELVES as forward bmm calls (with
    transposed-view operands — probed fault-free and faster than
    transpose copies, tests/moe_bmm_layout_probe_gpu.py) dodges it
    while keeping one grouped GEMM launch per matmul instead of the
    per-expert 2D loop."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return torch.bmm(x, w)

    @staticmethod
    def backward(ctx, go):
        x, w = ctx.saved_tensors
        go = go.contiguous()
        # transposed VIEWS where the layout is safe (probed per-GEMM in
        # tests/moe_bmm_layout_probe_gpu.py): the ONE faulting hipBLASLt
        # config on this stack is NT with a narrow inner dim
        # ([E,C,1024] @ [E,1024,4096]-view) — exactly gx of the second
        # expert linear; that operand alone gets a contiguous copy
        # (~175 us/layer) while the other three GEMMs ride views
        wt = w.transpose(1, 2)
        if wt.shape[-1] > wt.shape[-2]:   # widening NT: the faulting one
            wt = wt.contiguous()
        gx = torch.bmm(go, wt)
        gw = torch.bmm(x.transpose(1, 2), go)
        return gx, gw


class ExpertParallelMLP(nn.Module):
    """num_experts split across the comm group; each rank holds
    num_experts // world experts (reference tests use the same layout,
    tests/split_test.py:30-90)."""

    def __init__(self, hidden, ffn_hidden, num_experts, comm=None, top_k=2,
                 capacity_factor=1.25, aux_loss_coef=0.0, z_loss_coef=0.0,
                 fused_router=None):
        """aux_loss_coef / z_loss_coef: weights of the load-balance loss
        L_bal and the router z loss L_z (module docstring) in the
        gradient; the step's reported loss stays the task loss.
        fused_router: None = the native router kernels whenever a
        coefficient is non-zero and they apply (native build, device
        tensor, bf16/fp32 logits, top_k <= 2, 2 <= num_experts <= 256);
        True / False force the choice, as EPL_MOE_FUSED_ROUTER=1/0 does
        for modules built with None."""
        super().__init__()
        self.aux_loss_coef = float(aux_loss_coef)
        self.z_loss_coef = float(z_loss_coef)
        self.fused_router = fused_router
        self.last_balance_loss = None
        self.last_z_loss = None
        self.last_expert_counts = None
        self.comm = comm
        self.world = comm.size if comm is not None else 1
        assert num_experts % self.world == 0, \
            "num_experts must divide the split degree"
        self.num_experts = num_experts
        self.ffn_hidden = ffn_hidden
        self.local_experts = num_experts // self.world
        self.hidden = hidden
        self.top_k = top_k
        self.capacity_factor = capacity_factor
        self.gate = nn.Linear(hidden, num_experts, bias=False)
        self.w1 = nn.Parameter(
            torch.empty(self.local_experts, hidden, ffn_hidden))
        self.w2 = nn.Parameter(
            torch.empty(self.local_experts, ffn_hidden, hidden))
        nn.init.normal_(self.w1, std=0.02)
        nn.init.normal_(self.w2, std=0.02)
        if self.world > 1:
            self.w1._epl_shard_dim = 0
            self.w2._epl_shard_dim = 0

    def set_comm(self, comm):
        """Called by the engine's split transform: shard the expert weights
        constructed with comm=None (full expert set) down to this rank's
        slice (reference: expert weights inside epl.split, hooks.py:758)."""
        if comm is None or comm.size == 1:
            self.comm = comm
            return
        assert self.world == 1, "expert weights already sharded"
        self.comm = comm
        self.world = comm.size
        assert self.num_experts % self.world == 0
        self.local_experts = self.num_experts // self.world
        shard = max(comm.rank, 0)
        lo = shard * self.local_experts
        hi = lo + self.local_experts
        with torch.no_grad():
            self.w1 = nn.Parameter(self.w1[lo:hi].clone())
            self.w2 = nn.Parameter(self.w2[lo:hi].clone())
        self.w1._epl_shard_dim = 0
        self.w2._epl_shard_dim = 0

    def _wire_compression(self):
        # reference parallel/ops.py:485-495: optional fp16 all-to-all;
        # only meaningful for fp32 activations (bf16 ships bf16 anyway)
        from easyparallellibrary_amd.env import Env
        return Env.get().config.communication.compression

    def _router_mode(self, x):
        """None: the original gating ops.  "torch" / "fused": the router
        of the module docstring, in torch ops or in the kernels."""
        has_aux = self.aux_loss_coef != 0.0 or self.z_loss_coef != 0.0
        want = self.fused_router
        if want is None:
            env = _moe_fused_router_env()
            if env in ("0", "1"):
                want = env == "1"
        if want is None:
            want = has_aux
        if want:
            can = (self.top_k <= 2 and ROUTER_MIN_EXPERTS
                   <= self.num_experts <= ROUTER_MAX_EXPERTS
                   and use_native(x))
            if can:
                return "fused"
            if self.fused_router:
                raise RuntimeError(
                    "fused_router=True needs the native extension, a "
                    "device tensor, top_k <= 2 and {} <= num_experts <= {}"
                    .format(ROUTER_MIN_EXPERTS, ROUTER_MAX_EXPERTS))
        return "torch" if has_aux else None

    def _route(self, x, mode):
        logits = self.gate(x)
        if mode == "fused" and logits.dtype in (torch.bfloat16,
                                                torch.float32):
            topi, topw, counts, l_bal, l_z = _FusedRouter.apply(
                logits, self.top_k)
        else:
            topi, topw, counts, l_bal, l_z = router_torch(logits,
                                                          self.top_k)
        self.last_balance_loss = l_bal.detach()
        self.last_z_loss = l_z.detach()
        self.last_expert_counts = counts
        return topi, topw, counts, l_bal, l_z

    def forward(self, x):
        orig_shape = x.shape
        x = x.reshape(-1, self.hidden)
        n_tokens = x.shape[0]
        mode = self._router_mode(x)
        counts = l_bal = l_z = None
        if mode is None:
            logits = self.gate(x).float()
            probs = logits.softmax(dim=-1)
            topv, topi = probs.topk(self.top_k, dim=-1)
            topv = topv / topv.sum(dim=-1, keepdim=True)
        else:
            topi, topv, counts, l_bal, l_z = self._route(x, mode)

        capacity = max(
            1, int(self.capacity_factor * n_tokens * self.top_k /
                   self.num_experts))
        flat_e = topi.reshape(-1)
        flat_t = (torch.arange(n_tokens, device=x.device)
                  .repeat_interleave(self.top_k))
        flat_w = topv.reshape(-1)
        # slot assignment per expert (ordered, capacity-dropped)
        order = torch.argsort(flat_e, stable=True)
        fe, ft, fw = flat_e[order], flat_t[order], flat_w[order]
        # position within expert via segmented arange.  scatter_add of
        # ones instead of bincount: bincount infers its output size on
        # the host (device sync), which both stalls the step and is
        # hipGraph-capture-unsupported; integer atomics make the
        # scatter_add exact and order-independent.
        if counts is None:
            counts = torch.zeros(self.num_experts, dtype=torch.long,
                                 device=x.device)
            counts.scatter_add_(0, fe, torch.ones_like(fe))
        seg_start = torch.nn.functional.pad(counts.cumsum(0), (1, 0))[:-1]
        pos_in_e = torch.arange(fe.numel(), device=x.device) - seg_start[fe]
        native = (_moe_native_dispatch() and use_native(x)
                  and x.dtype == torch.bfloat16 and self.hidden % 8 == 0)
        inv = None
        if native:
            # fused dispatch kernel: full assignment list, in-kernel
            # capacity skip — no boolean select / nonzero sync
            m = fe.numel()
            inv = torch.empty_like(order)
            inv[order] = torch.arange(m, device=x.device)
            dispatched = _MoEDispatch.apply(
                x, fe, pos_in_e, ft, inv, self.top_k, capacity,
                self.num_experts)
        else:
            keep = pos_in_e < capacity
            fe, ft, fw, pos_in_e = (fe[keep], ft[keep], fw[keep],
                                    pos_in_e[keep])
            # dispatch tensor: [num_experts, capacity, hidden]
            dispatched = x.new_zeros(self.num_experts, capacity,
                                     self.hidden)
            dispatched[fe, pos_in_e] = x[ft]

        # all-to-all: [world, local_experts*capacity, hidden]
        d = dispatched.reshape(self.world,
                               self.local_experts * capacity, self.hidden)
        if self.comm is not None and self.world > 1:
            d = functional.all_to_all(d.contiguous(), self.comm,
                                      compress=self._wire_compression())
        # now d[w] = tokens sent by rank w for MY local experts
        d = d.reshape(self.world, self.local_experts, capacity, self.hidden)
        d = d.transpose(0, 1).reshape(self.local_experts,
                                      self.world * capacity, self.hidden)
        # expert FFN: batched GEMM (one hipBLASLt grouped call per
        # matmul, hand-written backward above) by default; EPL_MOE_BMM=0
        # falls back to the per-expert 2D-GEMM loop
        if _moe_bmm():
            he = F.gelu(_BatchedExpertLinear.apply(d.contiguous(), self.w1))
            h = _BatchedExpertLinear.apply(he, self.w2)
        else:
            outs = []
            for e in range(self.local_experts):
                he = F.gelu(d[e] @ self.w1[e])
                outs.append(he @ self.w2[e])
            h = torch.stack(outs)
        h = h.reshape(self.local_experts, self.world, capacity, self.hidden)
        h = h.transpose(0, 1).reshape(
            self.world, self.local_experts * capacity, self.hidden)
        if self.comm is not None and self.world > 1:
            h = functional.all_to_all(h.contiguous(), self.comm,
                                      compress=self._wire_compression())
        h = h.reshape(self.num_experts, capacity, self.hidden)

        if native:
            out = _MoECombine.apply(h, fw, fe, pos_in_e, ft, inv,
                                    self.top_k, capacity, n_tokens)
        else:
            out = x.new_zeros(n_tokens, self.hidden)
            out.index_add_(0, ft,
                           h[fe, pos_in_e] * fw.unsqueeze(-1).to(h.dtype))
        if l_bal is not None:
            if self.aux_loss_coef != 0.0:
                out = _AttachAuxLoss.apply(out, l_bal, self.aux_loss_coef)
            if self.z_loss_coef != 0.0:
                out = _AttachAuxLoss.apply(out, l_z, self.z_loss_coef)
        return out.reshape(orig_shape)
