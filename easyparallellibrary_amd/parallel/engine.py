"""The parallel execution engine.

Capability parity: /root/reference/epl/parallel/parallel.py
(device_replacement :120-135, do_parallelism :211-231, merge_outputs
:233-353) + graph_editor.py (replica/micro-batch handling :389-443,
gradient aggregation :610-725).

MI355X redesign: no graph cloning.  Each rank instantiates the model once,
keeps only the taskgraphs (pipeline stage / shard) it owns, flattens their
parameters into device arenas (parallel/dp.py), and executes either the
plain forward (DP / TP) or the micro-batch pipeline schedule
(parallel/pipeline.py).  All gradient traffic is bucketed RCCL over xGMI,
overlapped with backward; the optimizer is one fused CDNA4 kernel per
arena (runtime/optim.py).
"""

import torch
import torch.distributed as dist
import torch.nn as nn

from easyparallellibrary_amd import constant
from easyparallellibrary_amd.cluster import Cluster, Layout
from easyparallellibrary_amd.comm.backend import create_communicator
from easyparallellibrary_amd.comm.pool import CommunicationPool
from easyparallellibrary_amd.env import Env
from easyparallellibrary_amd.ir.plan import Plan
from easyparallellibrary_amd.parallel.dp import FlatParamGroup, GradReducer
from easyparallellibrary_amd.runtime.optim import OPTIMIZERS
from easyparallellibrary_amd.utils.logging import get_logger

logger = get_logger()


class StageModule(nn.Module):
    """A pipeline stage: the taskgraph's maximal module roots run in
    registration order (the model must be stage-chainable — each stage
    output feeds the next stage, mirroring the reference's stage
    entrance/exit dataflow, ir/taskgraph.py:134-400)."""

    def __init__(self, modules):
        super().__init__()
        self.mods = nn.ModuleList(modules)

    def forward(self, x):
        for m in self.mods:
            x = m(x)
        return x


class Engine:
    _seq = 0

    def __init__(self, model, loss_fn=None, optimizer="adamw", lr=1e-3,
                 optimizer_kwargs=None, dtype=None):
        Engine._seq += 1
        self._ns = "e{}".format(Engine._seq)  # unique comm-name namespace
        self.env = Env.get()
        self.config = self.env.config
        self.env.get_or_create_process_group()
        self.cluster = Cluster()
        self.env.cluster = self.cluster
        self.device = self.cluster.device
        self.loss_fn = loss_fn
        self.dtype = dtype or torch.float32
        self.model = model
        from easyparallellibrary_amd.runtime.amp import AmpContext
        self.amp = AmpContext(self.config, self.device)
        if self.amp.enabled and self.dtype != torch.float32:
            raise ValueError(
                "amp.level=O1 keeps fp32 parameters; pass dtype=float32 "
                "(pure-bf16 training needs no AMP)")

        # ---- plan -----------------------------------------------------------
        if (self.config.auto.auto_parallel
                and not self.env.strategy_context.strategies):
            # reference hooks.py:130-134: auto mode tags the whole model
            # Replicate(1); auto-stage below then splits it if
            # pipeline.num_stages > 1
            from easyparallellibrary_amd.strategies.replicate import (
                Replicate)
            self.env.strategy_context.set_default_strategy(Replicate(1))
        self.plan = Plan.build(model, self.env.strategy_context)
        # auto-stage: partition an un-staged sequential model into
        # pipeline.num_stages stages (reference: parallel/planner.py
        # AutoStageGenerator, invoked from the gradients hook)
        auto_n = self.config.pipeline.num_stages
        if auto_n > 1 and self.plan.num_stages <= 1 \
                and not self.plan.has_split:
            from easyparallellibrary_amd.ir.plan import TaskGraph
            from easyparallellibrary_amd.parallel.planner import (
                AutoStageGenerator)
            from easyparallellibrary_amd.strategies.replicate import Replicate
            stages = AutoStageGenerator(model, auto_n).search()
            if stages is not None:
                tgs = []
                for i, mods in enumerate(stages):
                    strat = Replicate(1, name="auto_stage_{}".format(i))
                    strat.index = i
                    tg = TaskGraph(i, strat)
                    tg.modules = list(mods)
                    tg.module_names = [
                        "auto_stage_{}[{}]".format(i, j)
                        for j in range(len(mods))]
                    tgs.append(tg)
                self.plan = Plan(tgs, None)
                logger.info("auto-stage: partitioned model into %d stages "
                            "(%s modules per stage)", auto_n,
                            [len(m) for m in stages])
        colocate = self.config.cluster.colocate_split_and_replicate
        counts = self.plan.effective_device_counts(colocate)
        layout_counts = [c for c in counts if c > 0]
        if not layout_counts:
            layout_counts = [1]
        self.layout = Layout(self.cluster.world_size, layout_counts)
        vds = self.layout.slices()
        # assign virtual devices; colocated split tg shares the slice of the
        # preceding replicate tg with equal device_count
        vi = 0
        prev_by_count = {}
        for tg, c in zip(self.plan.taskgraphs, counts):
            if c == 0:
                tg.virtual_device = prev_by_count[tg.device_count]
            else:
                tg.virtual_device = vds[vi]
                vi += 1
                if not tg.is_split:
                    prev_by_count[tg.device_count] = tg.virtual_device

        self.rank = self.cluster.rank
        self.world_size = self.cluster.world_size
        self.per_replica = self.layout.per_replica
        self.replica_id = self.rank // self.per_replica
        self.num_replicas = self.layout.num_replicas

        # ---- control channel (object exchange; gloo works on GPU hosts too)
        self._control_group = None
        if dist.is_initialized() and dist.get_backend() != "gloo":
            self._control_group = dist.new_group(backend="gloo")

        # ---- stages ---------------------------------------------------------
        self.stage_tgs = [tg for tg in self.plan.taskgraphs
                          if tg.strategy_type == constant.REPLICATE]
        self.num_stages = len(self.stage_tgs) if len(self.stage_tgs) > 1 else 1
        self.my_stage = 0
        if self.num_stages > 1:
            # stage s of my replica runs on the tg's virtual-device ranks
            self.my_stage = None
            for s, tg in enumerate(self.stage_tgs):
                if self.rank in tg.virtual_device.local_ranks(self.replica_id):
                    self.my_stage = s
            assert self.my_stage is not None, (
                "rank {} owns no pipeline stage".format(self.rank))

        # ---- TP (split) transformation --------------------------------------
        self.tp_comm = None
        self._owned_tgs = []
        for tg in self.plan.taskgraphs:
            ranks = tg.virtual_device.local_ranks(self.replica_id)
            if self.rank in ranks:
                self._owned_tgs.append(tg)
        all_split_tgs = [tg for tg in self.plan.taskgraphs if tg.is_split]
        if all_split_tgs:
            from easyparallellibrary_amd.ops import split_transform
            for tg in all_split_tgs:
                for rep in range(self.num_replicas):
                    ranks = tg.virtual_device.local_ranks(rep)
                    mine = self.rank in ranks
                    if not mine and (torch.cuda.is_available()
                                     or not dist.is_initialized()):
                        continue  # RCCL init is group-local
                    comm = create_communicator(
                        "{}_tp_tg{}_rep{}".format(self._ns, tg.index, rep),
                        ranks)
                    if mine:
                        self.tp_comm = comm
                        split_transform.transform_taskgraph(tg, comm,
                                                            model=model)

        # ---- materialize my modules on device --------------------------------
        if self.num_stages > 1:
            self.stage_module = StageModule(self.stage_tgs[self.my_stage].modules)
            self._runnable = self.stage_module
        else:
            self._runnable = model
        for tg in self._owned_tgs:
            for m in tg.modules:
                m.to(self.device, dtype=self.dtype)

        # ---- gradient checkpointing (reference: runtime/gc/) ----------------
        gc_type = self.config.gradient_checkpoint.type
        self._gc_wrapped = 0
        if gc_type:
            from easyparallellibrary_amd.runtime.gc import (
                apply_gradient_checkpointing)
            end_tg = self.config.gradient_checkpoint.end_taskgraph
            allowed = None
            if end_tg >= 0:
                # restrict recompute to modules owned by taskgraphs with
                # index < end_taskgraph (reference gc end_taskgraph)
                allowed = set()
                for tg in self._owned_tgs:
                    if tg.index < end_tg:
                        for m in tg.modules:
                            allowed.update(id(sub) for sub in m.modules())
            n = apply_gradient_checkpointing(self._runnable, mode=gc_type,
                                             allowed=allowed)
            self._gc_wrapped = n
            logger.info("gradient checkpointing: wrapped %d module(s)", n)

        # ---- DP groups + reducers -------------------------------------------
        # Every rank must create communicators in the same global order
        # (gloo's new_group is collective).  Enumerate all (taskgraph,
        # position) DP groups deterministically.
        self.flat_groups = []
        self.reducers = []
        self._group_infos = []
        pool_n = self.config.communication.num_communicators
        bucket_bytes = self.config.communication.bucket_bytes
        reduce_method = self.config.communication.gradients_reduce_method
        overlap = self.config.communication.overlap_grad_reduce
        zero_level = self.config.zero.level
        self._bcast_jobs = []
        # ---- sparse-grad params (nn.Embedding(sparse=True)) -----------------
        # reference: rewriters/sparse_allreduce.py:39-173 + the
        # communication.sparse_as_dense knob (config.py:81).  Dense mode
        # keeps them in the arena (adopt_grad densifies); gather mode
        # excludes them and wires a SparseGradHandler per DP group.
        from easyparallellibrary_amd.parallel.sparse import (
            find_sparse_grad_params)
        self._sparse_ids = {
            id(p) for p in find_sparse_grad_params([self.model])}
        self._sparse_dense = self.config.communication.sparse_as_dense
        self.sparse_handlers = []
        _pending_sparse = []
        if self._sparse_ids and not self._sparse_dense and (
                zero_level or self.config.offload.level):
            raise ValueError(
                "sparse-grad embeddings with zero/offload need "
                "communication.sparse_as_dense=True (the gather-based "
                "sparse path keeps params outside the shard arenas)")
        for tg in self.plan.taskgraphs:
            vd = tg.virtual_device
            k = len(vd.local_ranks(0))
            if tg.is_split:
                # sharded params: DP group = shard i's copies across
                # replicas.  UN-sharded params inside a split scope (e.g.
                # the MoE gate) are replicated on every tg rank and sync
                # across all of them.
                groups = [
                    ([vd.local_ranks(r)[i] for r in range(self.num_replicas)],
                     "sharded", i)
                    for i in range(k)]
                groups.append((vd.all_ranks, "replicated", k))
            else:
                groups = [(vd.all_ranks, "all", 0)]
            my_pos = None
            ranks_here = vd.local_ranks(self.replica_id)
            if self.rank in ranks_here:
                my_pos = ranks_here.index(self.rank)
            for granks, kind, gi in groups:
                name = "{}_dp_tg{}_g{}".format(self._ns, tg.index, gi)
                if self.rank not in granks:
                    if not torch.cuda.is_available() and dist.is_initialized():
                        # gloo group creation is collective
                        CommunicationPool(name, granks, pool_n)
                        create_communicator(name + "_b", granks)
                    continue
                pool = CommunicationPool(name, granks, pool_n)
                bcomm = create_communicator(name + "_b", granks)
                params = [p for p in tg.parameters() if p.requires_grad]
                if kind == "sharded":
                    params = [p for p in params
                              if getattr(p, "_epl_shard_dim", None)
                              is not None]
                elif kind == "replicated":
                    params = [p for p in params
                              if getattr(p, "_epl_shard_dim", None) is None]
                if self._sparse_ids and not self._sparse_dense:
                    sp = [p for p in params if id(p) in self._sparse_ids]
                    params = [p for p in params
                              if id(p) not in self._sparse_ids]
                    if sp:
                        _pending_sparse.append((sp, bcomm, granks))
                if not params:
                    continue
                fg = FlatParamGroup(
                    params, self.device, model_dtype=self.dtype,
                    pad_to_multiple=len(granks) if zero_level else 1,
                    master_shard=((bcomm.rank, bcomm.size)
                                  if zero_level and bcomm is not None
                                  else None))
                reducer = GradReducer(
                    fg, pool, bucket_bytes, reduce_method=reduce_method,
                    overlap=overlap,
                    shard_owners=(zero_level == "v1"),
                    compression=self.config.communication.compression)
                self.flat_groups.append(fg)
                self.reducers.append(reducer)
                self._group_infos.append(
                    {"fg": fg, "pool": pool, "bcomm": bcomm,
                     "ranks": granks, "taskgraph": tg})
                self._bcast_jobs.append((fg, bcomm))

        # ---- initial weight sync (reference: hooks.py:330-357) ---------------
        for fg, bcomm in self._bcast_jobs:
            if bcomm is not None and bcomm.size > 1:
                bcomm.broadcast(fg.param_arena, root=0)
                fg.refresh_master()
        for sp, bcomm, _ in _pending_sparse:
            if bcomm is not None and bcomm.size > 1:
                for p in sp:
                    bcomm.broadcast(p.data, root=0)

        # ---- optimizer -------------------------------------------------------
        okw = dict(optimizer_kwargs or {})
        okw.setdefault("lr", lr)
        self.zero = None
        if self.config.zero.level:
            from easyparallellibrary_amd.runtime.zero import ZeroOptimizer
            self.optimizer = ZeroOptimizer(
                self, optimizer, okw, level=self.config.zero.level)
        elif self.config.offload.level:
            from easyparallellibrary_amd.runtime.offload import (
                CPUOffloadAdamW)
            if optimizer != "adamw":
                raise NotImplementedError("offload supports adamw")
            self.optimizer = CPUOffloadAdamW(self.flat_groups, **okw)
            n = self.optimizer.attach_reducers(
                self.reducers, [info["fg"] for info in self._group_infos])
            # eager CPU apply during backward needs the grad scale final
            # before backward ends: amp off, no global-norm clip
            self._offload_eager = bool(
                n and n == len(self.reducers) and not self.amp.enabled
                and not self.config.optimizer.max_grad_norm)
            if n:
                logger.info("offload: per-bucket D2H overlap on %d "
                            "reducer(s)%s", n,
                            " + eager CPU apply" if self._offload_eager
                            else "")
        else:
            self.optimizer = OPTIMIZERS[optimizer](self.flat_groups, **okw)
        for sp, bcomm, granks in _pending_sparse:
            from easyparallellibrary_amd.parallel.sparse import (
                SparseGradHandler)
            h = SparseGradHandler(
                sp, bcomm, reduce_method=reduce_method,
                lr=okw.get("lr", lr), betas=okw.get("betas", (0.9, 0.999)),
                eps=okw.get("eps", 1e-8),
                weight_decay=okw.get("weight_decay", 0.01))
            h.n_copies = max(1, len(granks))
            self.sparse_handlers.append(h)
        if self.sparse_handlers:
            logger.info("sparse-grad path: %d param(s) on the gather wire "
                        "(communication.sparse_as_dense=False)",
                        sum(len(h.params) for h in self.sparse_handlers))

        # ---- pipeline runtime ------------------------------------------------
        self.pipeline = None
        if self.num_stages > 1:
            from easyparallellibrary_amd.parallel.pipeline import (
                PipelineRuntime)
            self.pipeline = PipelineRuntime(self)

        # ---- PreferBackwardOptimizer: bucket-wise eager apply ---------------
        # (reference scheduler.py:87-116).  Gated to the plain fused-
        # AdamW path: eager applies cannot precede a found_inf check or
        # global grad-norm clip, and sharded owners/compression change
        # when a bucket's grads are final in the arena.
        from easyparallellibrary_amd.runtime.optim import FusedAdamW
        self._pbo_eager = False
        if (self.pipeline is not None
                and self.config.pipeline.strategy
                == constant.SCHEDULER_PREFER_BACKWARD_OPT
                and type(self.optimizer) is FusedAdamW
                and not self.amp.enabled
                and not self.config.optimizer.max_grad_norm
                and not zero_level and not self.config.offload.level
                and not self.sparse_handlers
                and all(r.supports_bucket_callbacks and not r.shard_owners
                        for r in self.reducers)):
            def _mk(fg):
                def cb(bi, lo, hi, comm, owner):
                    self.optimizer.eager_apply(fg, lo, hi, comm)
                return cb
            for red, info in zip(self.reducers, self._group_infos):
                red.on_bucket_reduced = _mk(info["fg"])
            self._pbo_eager = True
            logger.info("prefer_backward_optimizer: eager bucket apply "
                        "on %d reducer(s)", len(self.reducers))

        self.global_step = 0
        self._accum_count = 0
        # hipGraph-captured simple step (runtime/hipgraph.py): None =
        # requested, eligibility checked lazily at the first step (GC
        # wrapping happens after __init__); False = off/ineligible
        self._hipgraph = None if self.config.kernel.hip_graph else False
        logger.info(
            "Engine ready: world=%d stages=%d replicas=%d per_replica=%d "
            "dtype=%s groups=%d", self.world_size, self.num_stages,
            self.num_replicas, self.per_replica, self.dtype,
            len(self.flat_groups))

    # ---- helpers -------------------------------------------------------------
    @property
    def num_micro_batch(self):
        return max(1, self.config.pipeline.num_micro_batch)

    def _set_reducers_enabled(self, flag):
        for r in self.reducers:
            r.enabled = flag

    def finish_grad_sync(self):
        for r in self.reducers:
            r.finish()
        for h in self.sparse_handlers:
            h.reduce()

    def zero_grad(self):
        for fg in self.flat_groups:
            fg.zero_grad()
        for h in self.sparse_handlers:
            h.zero_grad()

    def forward(self, x):
        """Plain forward (this rank's stage under pipeline parallelism —
        see ``eval_step``)."""
        return self._runnable(x)

    # ---- the training step ---------------------------------------------------
    def train_step(self, inputs, targets, accumulate=False):
        """One optimizer step: micro-batch loop (pipeline or GA), overlapped
        DP gradient reduction, fused optimizer.  Returns the local mean loss
        tensor (on the last stage; None elsewhere for pipelines).

        ``accumulate=True`` runs forward+backward only (no reduction, no
        optimizer) so callers can drive their own accumulation loop; the
        next ``accumulate=False`` call reduces everything accumulated and
        steps once, dividing by the number of accumulated calls."""
        # MoE aux losses inject their gradient inside backward: it has to
        # carry the loss scale of this step (constant within a step)
        from easyparallellibrary_amd.ops.moe import set_aux_loss_scale
        set_aux_loss_scale(self.amp.loss_scale)
        if accumulate:
            if self.pipeline is not None:
                raise ValueError(
                    "manual accumulation is not supported with pipeline "
                    "parallelism (use pipeline.num_micro_batch)")
            if self._accum_count == 0:
                self.zero_grad()
            self._set_reducers_enabled(False)
            with self.amp.autocast():
                loss = self.loss_fn(self._runnable(inputs), targets)
            self.amp.scale_loss(loss).backward()
            self._accum_count += 1
            return loss.detach()
        if self._accum_count == 0:
            self.zero_grad()
        if self._pbo_eager:
            # grad scale is known before backward (amp off, no manual
            # accumulation under pipeline): buckets apply as they reduce
            self.optimizer.begin_eager(float(self.num_micro_batch))
        if getattr(self, "_offload_eager", False) and not (
                self._gc_wrapped
                and self.config.gradient_checkpoint.check_gradients
                and self.global_step == 0):
            # same precondition as PBO: scale final before backward
            self.optimizer.begin_step(
                float(self.num_micro_batch) * (self._accum_count + 1))
        if self.pipeline is not None:
            loss = self.pipeline.run(inputs, targets)
        elif self._hipgraph is not False:
            if self._hipgraph is None:   # lazy first-step eligibility
                from easyparallellibrary_amd.runtime import hipgraph
                ok, reason = hipgraph.eligible(self)
                if ok:
                    self._hipgraph = hipgraph.HipGraphStep(self)
                else:
                    logger.info("kernel.hip_graph requested but the step "
                                "is not capture-safe: %s — running eager",
                                reason)
                    self._hipgraph = False
            if self._hipgraph is not False:
                loss = self._hipgraph.run(inputs, targets)
            else:
                loss = self._train_step_simple(inputs, targets)
        else:
            loss = self._train_step_simple(inputs, targets)
        if (self._gc_wrapped
                and self.config.gradient_checkpoint.check_gradients
                and self.global_step == 0):
            self._verify_gc_gradients(inputs, targets)
        found_inf = self.amp.found_inf(self.flat_groups)
        n_accum = self._accum_count + 1
        self._accum_count = 0
        if not found_inf:
            grad_scale = (float(self.num_micro_batch) * n_accum
                          * self.amp.loss_scale)
            max_norm = self.config.optimizer.max_grad_norm
            if max_norm:
                gnorm = self._global_grad_norm() / grad_scale
                if gnorm > max_norm:
                    # shrink by gnorm/max_norm via the optimizer's fused
                    # unscale — no extra pass over the arenas
                    grad_scale *= gnorm / max_norm
            self.optimizer.step(grad_scale=grad_scale)
            for h in self.sparse_handlers:
                h.step(grad_scale=grad_scale)
        self.amp.post_step(found_inf)
        self.global_step += 1
        return loss

    def _verify_gc_gradients(self, inputs, targets):
        """One-time self-check (reference gc check_gradients,
        gradient_checkpoint.py:310-325): recompute the first step's
        gradients with recompute disabled and log the max deviation;
        the checkpointed gradients are kept for the actual step."""
        from easyparallellibrary_amd.runtime.gc import CheckpointWrapper
        snap = [fg.grad_arena.clone() for fg in self.flat_groups]
        wrappers = [m for m in self._runnable.modules()
                    if isinstance(m, CheckpointWrapper)]
        for w in wrappers:
            w.enabled = False
        # suppress bucket callbacks for the verification rerun (eager
        # PBO applies / offload D2H must not fire on throwaway grads)
        saved_cbs = [r.on_bucket_reduced for r in self.reducers]
        for r in self.reducers:
            r.on_bucket_reduced = None
        self.zero_grad()
        if self.pipeline is not None:
            # collective: every pipeline rank reruns the schedule with
            # recompute off and compares its local stage's gradients
            self.pipeline.run(inputs, targets)
        else:
            self._train_step_simple(inputs, targets)
        worst = 0.0
        for fg, s0 in zip(self.flat_groups, snap):
            worst = max(worst, float(
                (fg.grad_arena.float() - s0.float()).abs().max()))
        logger.info("gc check_gradients: max |gc - plain| grad deviation "
                    "= %.3e", worst)
        for w in wrappers:
            w.enabled = True
        for r, cb in zip(self.reducers, saved_cbs):
            r.on_bucket_reduced = cb
        for fg, s0 in zip(self.flat_groups, snap):
            fg.grad_arena.copy_(s0)

    def set_lr(self, lr):
        """Update the learning rate for subsequent steps (schedules are
        the caller's loop; the fused optimizers read ``lr`` each step)."""
        opt = self.optimizer
        inner = getattr(opt, "inner", None)
        (inner if inner is not None else opt).lr = float(lr)
        for h in self.sparse_handlers:
            h.lr = float(lr)

    @property
    def lr(self):
        opt = self.optimizer
        inner = getattr(opt, "inner", None)
        return (inner if inner is not None else opt).lr

    def _global_grad_norm(self):
        """Global L2 norm of the de-duplicated gradient: each arena's
        ||g||^2 is divided by its DP-group size (the number of ranks
        holding an identical copy) and summed over the world, so every
        unique parameter counts exactly once across DP replicas,
        pipeline stages and TP/EP shards (reference capability:
        communication.clip_after_allreduce, epl/config.py:96-97)."""
        from easyparallellibrary_amd.ops.dispatch import (native_ext,
                                                          use_native)
        total = torch.zeros(1, dtype=torch.float32, device=self.device)
        for info, red in zip(self._group_infos, self.reducers):
            g = info["fg"].grad_arena
            n_copies = max(1, len(info["ranks"]))
            if red.shard_owners and n_copies > 1:
                # ZeRO v1: only my shard's slice holds fully reduced
                # grads (the rest is unreduced partials) — count it once
                shard = info["fg"].total // n_copies
                r = info["bcomm"].rank
                g = g[r * shard:(r + 1) * shard]
                n_copies = 1
            if use_native(g):
                sq = torch.zeros(1, dtype=torch.float32, device=g.device)
                native_ext().sqnorm(g, sq)
            else:
                sq = g.float().pow(2).sum().reshape(1)
            total += sq / n_copies
        for h in self.sparse_handlers:
            total += h.sqnorm().to(total.device) / h.n_copies
        if dist.is_initialized():
            use_dev = (dist.get_backend() == "nccl"
                       and self.device.type == "cuda")
            t = total if use_dev else total.cpu()
            dist.all_reduce(t)
            total = t
        return float(total.sqrt())

    def _train_step_simple(self, inputs, targets):
        nmb = self.num_micro_batch
        if nmb > 1:
            input_chunks = torch.chunk(inputs, nmb, dim=0)
            target_chunks = torch.chunk(targets, nmb, dim=0)
        else:
            input_chunks = [inputs]
            target_chunks = [targets]
        total_loss = None
        for i, (xc, tc) in enumerate(zip(input_chunks, target_chunks)):
            last = (i == nmb - 1)
            self._set_reducers_enabled(last)
            with self.amp.autocast():
                out = self._runnable(xc)
                loss = self.loss_fn(out, tc)
            self.amp.scale_loss(loss).backward()
            total_loss = loss.detach() if total_loss is None \
                else total_loss + loss.detach()
        self.finish_grad_sync()
        return total_loss / nmb

    # ---- eval ----------------------------------------------------------------
    def eval_step(self, inputs):
        """Forward in eval mode without grad (dropout off, BatchNorm uses
        running stats and does not update them).  Under pipeline
        parallelism this runs the PIPELINED forward chain — collective
        across the replica's stages; stage 0 consumes ``inputs``, the
        last stage returns the outputs, other stages return None
        (PipelineRuntime.run_eval)."""
        if self.pipeline is not None:
            return self.pipeline.run_eval(inputs)
        was_training = self._runnable.training
        self._runnable.eval()
        try:
            with torch.no_grad():
                return self._runnable(inputs)
        finally:
            self._runnable.train(was_training)

    # ---- merged outputs (reference: parallel/parallel.py:233-353) ------------
    def all_reduce_metric(self, value, op="mean"):
        """Merge a scalar/tensor metric across every rank (the reference's
        merged loss/metric collections).  Returns the merged tensor."""
        t = value if torch.is_tensor(value) else torch.tensor(
            float(value), device=self.device)
        t = t.detach().clone()
        if not dist.is_initialized() or self.world_size == 1:
            return t
        if t.is_cuda and dist.get_backend() == "nccl":
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
        else:
            tc = t.cpu()
            dist.all_reduce(tc, op=dist.ReduceOp.SUM,
                            group=self._control_group)
            t = tc.to(t.device)
        if op == "mean":
            t = t / self.world_size
        return t

    def merged_collections(self):
        """Merge the GLOBAL_* collections across ranks (reference:
        parallel/parallel.py merge_outputs :233-353: allgather/allreduce of
        user-collected losses/metrics)."""
        import easyparallellibrary_amd as epl
        out = {}
        env = self.env
        for name, op in ((epl.GraphKeys.GLOBAL_MEAN_OBJECTS, "mean"),
                         (epl.GraphKeys.GLOBAL_SUM_OBJECTS, "sum")):
            vals = env.get_collection(name)
            if vals:
                out[name] = [self.all_reduce_metric(v, op=op) for v in vals]
        concat = env.get_collection(epl.GraphKeys.GLOBAL_CONCAT_OBJECTS)
        if concat:
            from easyparallellibrary_amd.comm import functional
            from easyparallellibrary_amd.comm.backend import (
                create_communicator)
            comm = create_communicator(
                "{}_concat".format(self._ns), list(range(self.world_size)))
            out[epl.GraphKeys.GLOBAL_CONCAT_OBJECTS] = [
                functional.all_gather(
                    (v if torch.is_tensor(v) else torch.tensor(v))
                    .detach().reshape(1, -1).contiguous(), comm)
                for v in concat]
        for name in (epl.GraphKeys.LOCAL_MEAN_OBJECTS,
                     epl.GraphKeys.LOCAL_SUM_OBJECTS,
                     epl.GraphKeys.LOCAL_CONCAT_OBJECTS):
            vals = env.get_collection(name)
            if vals:
                out[name] = vals
        return out

    def broadcast_signal(self, value=0.0, root=0):
        """Broadcast a scalar from ``root`` to every rank — the
        reference's eval-barrier sync signal (hooks.py:915-933: workers
        block on a broadcast until the chief finishes evaluation).
        COLLECTIVE when world>1: acts as a barrier; returns the root's
        value as a float on every rank."""
        t = torch.tensor(float(value))
        if dist.is_initialized() and self.world_size > 1:
            dist.broadcast(t, root, group=self._control_group)
        return float(t)

    def write_summaries(self, writer, step, scalars=None):
        """Merge scalar summaries across every rank (mean) and write them
        on rank 0 — the reference rewires ``tf.summary`` inputs to the
        replica-merged tensors so TensorBoard shows whole-job values
        (parallel/parallel.py:355-413, §5 observability); here the engine
        merges at write time instead of editing a graph.

        COLLECTIVE when world>1: every rank must call it each step.
        ``scalars`` is a per-step dict name->value; additionally every
        ``(name, value_or_callable)`` registered once via
        ``epl.add_to_collection((name, fn), GraphKeys.SUMMARIES)`` is
        evaluated (callables play the role of the reference's live graph
        tensors).  ``writer`` is duck-typed — a
        ``torch.utils.tensorboard.SummaryWriter`` or anything with an
        ``add_scalar(name, value, step)`` method; it may be None on
        ranks that do not write.  Returns the merged {name: float}."""
        import easyparallellibrary_amd as epl
        items = list((scalars or {}).items())
        for entry in self.env.get_collection(epl.GraphKeys.SUMMARIES):
            name, v = entry
            items.append((name, v() if callable(v) else v))
        merged = {}
        for name, v in items:
            merged[name] = float(self.all_reduce_metric(v, op="mean"))
        if self.rank == 0 and writer is not None:
            for name, v in merged.items():
                writer.add_scalar(name, v, step)
        return merged

    def slice_input_files(self, files):
        """Per-replica IO slicing (config io.slicing; reference
        graph_editor.py:149-215)."""
        from easyparallellibrary_amd.utils.io_slicing import slice_files
        return slice_files(files, self.num_replicas, self.replica_id,
                           unbalanced=self.config.io.unbalanced_io_slicing,
                           drop_last=self.config.io.drop_last_files)

    # ---- replica consistency -------------------------------------------------
    def check_param_consistency(self):
        """Detect silent parameter drift between ranks that hold
        replicated copies (nondeterministic GPU kernels can desync e.g.
        the positions of a wide pipeline stage over many steps —
        advisor finding r1).  COLLECTIVE.  Returns the worst absolute
        checksum deviation across all replicated groups."""
        worst = 0.0
        for info in self._group_infos:
            if len(info["ranks"]) <= 1:
                continue
            fg, bcomm = info["fg"], info["bcomm"]
            local = fg.param_arena.to(torch.float64).sum().reshape(1)
            local = local.to(torch.float32)
            if fg.param_arena.is_cuda:
                out = torch.empty(bcomm.size, dtype=torch.float32,
                                  device=fg.param_arena.device)
                bcomm.all_gather(out, local.to(fg.param_arena.device))
            else:
                out = torch.empty(bcomm.size, dtype=torch.float32)
                bcomm.all_gather(out, local)
            dev = float((out - out[0]).abs().max())
            worst = max(worst, dev)
        if worst > 0:
            logger.warning(
                "replicated parameters drifted across ranks (max checksum "
                "delta %.3e) — call engine.resync_params()", worst)
        return worst

    def resync_params(self):
        """Force bitwise consistency of replicated parameters: broadcast
        every group's arena from its rank 0 and refresh fp32 masters.
        COLLECTIVE; use at checkpoint/eval points if
        check_param_consistency reported drift."""
        for fg, bcomm in self._bcast_jobs:
            if bcomm is not None and bcomm.size > 1:
                bcomm.broadcast(fg.param_arena, root=0)
                fg.refresh_master()

    # ---- teardown ------------------------------------------------------------
    def close(self):
        """Release this engine's resources: autograd hooks and every
        communicator created under its namespace (RCCL comms + HIP
        streams are destroyed; the global registry shrinks).  The engine
        must not be used afterwards.  COLLECTIVE-free."""
        for r in self.reducers:
            r.remove_hooks()
        ex = getattr(self.optimizer, "_eager_exec", None)
        if ex is not None:
            ex.shutdown(wait=True)
        from easyparallellibrary_amd.comm.backend import destroy_namespace
        n = destroy_namespace(self._ns + "_")
        logger.info("engine %s closed: %d communicator(s) destroyed",
                    self._ns, n)

    # ---- checkpoint ----------------------------------------------------------
    def save_checkpoint(self, path, save_optimizer=True):
        from easyparallellibrary_amd.runtime import saver
        # mixed-width stages replicate params across positions with no
        # per-step sync; surface any nondeterministic-kernel drift at
        # checkpoint time (advisor r1) — warn-only, collective
        if any(getattr(tg, "replicated_io", False)
               for tg in self.plan.taskgraphs):
            self.check_param_consistency()
        saver.save_checkpoint(self, path, save_optimizer=save_optimizer)

    def load_checkpoint(self, path, load_optimizer=True, assign_map=None,
                        strict=True):
        from easyparallellibrary_amd.runtime import saver
        saver.load_checkpoint(self, path, load_optimizer=load_optimizer,
                              assign_map=assign_map, strict=strict)
        meta = saver.ShardingLoader(path).meta
        self.global_step = meta.get("global_step", 0)
        scale = meta.get("amp_loss_scale")
        if scale is not None and self.amp.enabled:
            self.amp.scaler.scale = float(scale)
