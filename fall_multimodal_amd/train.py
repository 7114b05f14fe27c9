"""Fused training step: forward -> soft-target CE -> backward -> (all-reduce) -> optimizer
(RMSprop by default; SGD / Adam / AdamW, weight decay and global grad-norm clipping through
TrainStep(optimizer=..., max_norm=...), model/optimizer.py:8-35, root main.py:108-113).

This is the reference's inner loop body (Multimodal_Fall3/model/main.py:97-132; notebook
GSTCAN_HAR_conv_10kfold.ipynb:1103-1116) as native calls on one HIP stream with every
buffer preallocated, so it can be captured into HIP graphs and replayed per batch.

Data parallel: one process per GPU. Gradients live in ONE flat fp32 buffer whose layout
puts the parameters the first backward phase finalises (head, sensor branch, skeleton
layers 4-6; f3_net_grad_split) first. Phase 1 returns without joining its private queues:
the head bucket's all-reduce (RCCL, sum) is issued from a side stream that waits on phase
1's per-queue events (f3_net_wait_phase1), so phase 2's critical path (layers 0-3, data_bn)
starts at once while phase 1's weight gradients drain and the all-reduce runs; the remainder
follows phase 2. 1/world is applied inside the RMSprop kernel. BatchNorm statistics stay
per-rank (the reference's per-device batch semantics).
"""
from __future__ import annotations

import contextlib
import ctypes
import os

import numpy as np
import torch
import torch.distributed as dist

from . import metrics as _metrics, ops, optim as _optim
from ._flat import grad_views
from ._lib import ENTRY_PARAM, check, lib, ptr, stream_handle


class GradSync:
    """Two-bucket gradient all-reduce over a flat buffer: `head` = grads[:split] (final after
    backward phase 1), `tail` = grads[split:]. Both are issued async; `finish()` orders the
    caller's stream after them. `wait_phase1(stream_handle)` (optional) makes a stream wait for
    the phase-1 gradients: the head bucket is then issued from a side stream ordered after them
    rather than after everything on the caller's stream."""

    def __init__(self, grads: torch.Tensor, split: int, group=None, wait_phase1=None, force=False):
        self.grads, self.split, self.group = grads, int(split), group
        self.world = dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1
        self.wait_phase1 = wait_phase1
        # force: issue both buckets even at world 1 (a world-1 sum is the identity), so the collective
        # path runs on a one-GPU box (tests/test_gpu_rccl.py); needs an initialised process group
        self.active = self.world > 1 or bool(force)
        # high priority: ROCm draws high-priority streams from their own hardware-queue pool, so the head
        # bucket's wait + all-reduce never queue behind main-chain kernels on a shared normal-priority
        # queue (the step's four native queues already fill GPU_MAX_HW_QUEUES = 4)
        self._side = (torch.cuda.Stream(device=grads.device, priority=-1) if (self.active and grads.is_cuda)
                      else None)
        self._work = []

    def _reduce(self, t):
        if t.numel():
            self._work.append(dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group, async_op=True))

    def start_head(self, after_current=False):
        """after_current: order the bucket after everything on the caller's stream (a replayed
        graph, whose phase 1 joined its queues) instead of after phase 1's per-queue events."""
        if not self.active:
            return
        if after_current and self._side is not None:
            self._side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self._side):
                self._reduce(self.grads[:self.split])
            return
        if self.wait_phase1 is None or self._side is None:
            self._reduce(self.grads[:self.split])
            return
        self.wait_phase1(ctypes.c_void_p(self._side.cuda_stream))
        with torch.cuda.stream(self._side):
            self._reduce(self.grads[:self.split])

    def start_tail(self):
        if self.active:
            self._reduce(self.grads[self.split:])

    def finish(self):
        for w in self._work:
            w.wait()
        self._work = []

    def all(self):
        self.start_head()
        self.start_tail()
        self.finish()


def rccl_options():
    """ProcessGroupNCCL options for the gradient all-reduce: RCCL's internal stream high priority, for
    the same reason as GradSync's side stream (pass as init_process_group("nccl", pg_options=...))."""
    o = dist.ProcessGroupNCCL.Options()
    o.is_high_priority_stream = True
    return o


def check_step_args(label_smoothing=0.0, accum_iter=1):
    """TrainStep's checks of its two loop settings (no device needed): label_smoothing a number in
    [0, 1] (torch.nn.CrossEntropyLoss's range), accum_iter an integer >= 1. Returns (float, int)."""
    if isinstance(label_smoothing, bool) or not isinstance(label_smoothing, (int, float, np.integer, np.floating)):
        raise ValueError(f"TrainStep: label_smoothing must be a number in [0, 1], got {label_smoothing!r}")
    if not 0.0 <= float(label_smoothing) <= 1.0:  # (a NaN fails both comparisons)
        raise ValueError(f"TrainStep: label_smoothing must be in [0, 1], got {label_smoothing!r}")
    if isinstance(accum_iter, bool) or not isinstance(accum_iter, (int, np.integer)) or accum_iter < 1:
        raise ValueError(f"TrainStep: accum_iter must be an integer >= 1, got {accum_iter!r}")
    return float(label_smoothing), int(accum_iter)


def check_class_weight(w, num_class):
    """TrainStep's check of its class weights (no device needed): a sequence, ndarray or tensor of exactly
    `num_class` real numbers, each finite and >= 0 and not all zero (torch.nn.CrossEntropyLoss(weight=w)
    with a weight it can divide by). Returns a float32 ndarray [num_class]; anything else raises ValueError."""
    if isinstance(w, torch.Tensor):
        w = w.detach().cpu().numpy()
    if isinstance(w, (str, bytes)) or w is None:
        raise ValueError(f"class_weight must be {num_class} real numbers, got {w!r}")
    try:
        a = np.asarray(w)
    except Exception as e:  # a ragged sequence
        raise ValueError(f"class_weight must be {num_class} real numbers, got {w!r}") from e
    if a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.integer) or np.issubdtype(a.dtype, np.floating)):
        raise ValueError(f"class_weight must be {num_class} real numbers, got dtype {a.dtype}")
    if a.shape != (int(num_class),):
        raise ValueError(f"class_weight must have shape ({int(num_class)},), got {a.shape}")
    a = a.astype(np.float64)
    if not np.isfinite(a).all() or (a < 0).any():
        raise ValueError(f"class_weight must be finite and >= 0, got {a.tolist()}")
    with np.errstate(over="ignore"):
        a32 = a.astype(np.float32)
    if not np.isfinite(a32).all() or not (a32 > 0).any():
        raise ValueError(f"class_weight must be finite in float32 and not all zero, got {a.tolist()}")
    return a32


def check_ema_decay(ema_decay):
    """TrainStep's check of its averaging setting (no device needed): a number in [0, 1], the range in which
    get_ema_multi_avg_fn's lerp stays between the average and the parameters. Returns the float."""
    if isinstance(ema_decay, bool) or not isinstance(ema_decay, (int, float, np.integer, np.floating)):
        raise ValueError(f"TrainStep: ema_decay must be a number in [0, 1], got {ema_decay!r}")
    if not 0.0 <= float(ema_decay) <= 1.0:  # (a NaN fails both comparisons)
        raise ValueError(f"TrainStep: ema_decay must be in [0, 1], got {ema_decay!r}")
    return float(ema_decay)


def accum_updates(num_batches, accum_iter):
    """Which batches of an epoch end with optimizer.step() and model.zero_grad(): the reference's
    test `i % accum_iter == 0 or i + 1 == len(dataloader)` with i counted from the epoch's start
    (model/main.py:115-132). So batch 0 updates alone, then every accum_iter-th batch, then the last."""
    _, k = check_step_args(0.0, accum_iter)
    n = int(num_batches)
    return [i % k == 0 or i + 1 == n for i in range(n)]


def step_kwargs(config):
    """TrainStep's keyword arguments that the reference's loop reads from TRAIN.* (model/main.py:280
    LABEL_SMOOTHING, :115-132 ACCUM_ITER; root main.py:108-113 MAX_NORM)."""
    t = config.TRAIN
    return {"max_norm": t.MAX_NORM, "label_smoothing": t.LABEL_SMOOTHING, "accum_iter": t.ACCUM_ITER}


class TrainStep:
    """`optimizer` (optional, e.g. fall3 RMSprop driven by a CosineLRScheduler): its
    param_groups[0] lr / alpha / eps are read at every step, so a scheduler's step(epoch) takes
    effect as with the reference's optimizer.step() (model/main.py:127, 321-322). A captured step
    follows them too: its optimizer graph reads lr, alpha, eps, momentum, betas, weight_decay, max_norm and
    1/world from a device block (`hyper`; ops.hyper_views) that every call rewrites when one of them has
    changed, with one small launch before the replay and none otherwise. What the graph fixes is the
    step's structure (optim.hyper_structure: the kind, nesterov, momentum zero or not, plain RMSprop or
    not, clipping on or off); a call after one of those changed raises ValueError: capture() again.

    The optimizer's class picks the update: f3.RMSprop / SGD / Adam / AdamW (or torch.optim's), with the
    hyper-parameters of its param_groups[0] (momentum, nesterov, betas, weight_decay, ...), also read at
    every step. `max_norm` (TRAIN.MAX_NORM) clips the global L2 gradient norm as clip_grad_norm_ does
    (root main.py:108-113): the coefficient is applied inside the update, self.grads stays unscaled, and
    `grad_norm` / `clip_coef` are 1-element device tensors of the last step (no host sync). RMSprop
    without weight decay or clipping (the default, and what bench.py measures) runs exactly the
    launches it always did (f3_net_backward_rmsprop / f3_rmsprop_step); everything else runs
    f3_net_backward_optim / f3_optim_step. The states live in flat buffers (`square_avg`;
    `momentum_buffer`; `exp_avg`, `exp_avg_sq`) and the step count on the device (`step_count`), so a
    captured step advances it; optimizer_state_dict() / load_optimizer_state_dict() convert to and
    from torch's state_dict layout (model/main.py:302, 336).

    `metrics` (a metrics.StepMetrics, or True for one with top_k=(1,)): every step adds its batch's loss,
    top-k hits and confusion counts to the device accumulators with one launch directly after the loss
    (model/main.py:134-135 without the copy to the host), eager or replayed; capture() leaves them as
    they were. None (the default) issues exactly the launches the step always issued.
    param_grad_norms() gives the per-parameter gradient norms of model/main.py:84-89 without a sync.

    `label_smoothing` (TRAIN.LABEL_SMOOTHING, model/main.py:280): above 0 the loss launch is
    f3_net_loss_ex; `loss`, `dout` and the metrics' loss are the smoothed ones (the reference logs the
    smoothed loss), ranks and confusion counts come from the unsmoothed label. At 0.0 (the default) the
    step issues f3_net_loss as ever.

    `class_weight` (torch.nn.CrossEntropyLoss(weight=w), the usual first remedy for an imbalanced label set;
    data.class_weights gives sklearn's "balanced" ones): `num_class` finite numbers >= 0, not all zero
    (check_class_weight), kept in a device f32[C] tensor. The loss launch is then f3_net_loss_w, with
    `label_smoothing` as given, 0 included; `loss`, `dout` and the metrics' loss are the weighted ones, ranks
    and confusion counts are unchanged. prepare() turns 1-D labels into one-hot rows as the reference's loop
    does (model/main.py:104-113), so the step ALWAYS applies torch's rule for probability targets: the sum of
    w_c y'_c lsm_c over the batch divided by N. With non-uniform weights that is not what torch computes for
    class-index targets, which divides by the sum of the rows' weights instead (evaluate.valid_device with
    1-D labels is the one path that applies that rule). The divisor is N on every rank, so data parallelism
    and accum_iter need nothing new. `step.class_weight` returns a copy; setting it validates the value and
    copies it into the device tensor in place (eager, never inside a capture): the launch reads the weights
    when it runs, so a captured step follows the change on its next replay. Setting it on a step built with
    None, or to None, raises ValueError (the graph holds another launch). None (the default): no buffer and
    exactly the launches the step always issued.

    `accum_iter` (TRAIN.ACCUM_ITER, model/main.py:115-132): above 1 every call runs forward, loss and the
    whole backward into `grads`, then adds `grads` into the flat `accum` (f3_grad_accumulate; the first
    micro-batch after an update overwrites), and only update calls all-reduce `accum` and run the flat
    optimizer update on it, whatever the optimizer, with weight decay and clipping; `grad_norm` and
    `clip_coef` are those of the accumulated gradient, and p.grad / param_grad_norms() show `accum`.
    Which calls update follows the reference's rule (accum_updates) from begin_epoch(num_batches) on, or
    `update=True / False` per call; `pending` counts the micro-batches in `accum`, zero_grad() discards
    them. steps_taken() and the checkpoint count updates. At 1 (the default) nothing changes: no `accum`,
    the same launches, the per-layer fused update included.

    `skip_nonfinite` (what GradScaler.step does for an fp32 run, model/main.py:281): True applies the
    optimizer update of a call if and only if every element of the gradient it consumes (`grads`, or
    `accum` on an update call, after the all-reduce) is finite; otherwise the parameters, every state
    buffer and the device step count keep their bits. The decision is taken on the device from the fp64
    sum of squares (include/fall3.h), with no host sync, eager or replayed. `skipped` (int64) and
    `last_skipped` (int32) are 1-element device views, skipped_steps() the host count (a sync); after a
    skip `clip_coef` is 0 and `grad_norm` inf or NaN, after an applied step `grad_norm` is the norm even
    without max_norm. steps_taken() and the checkpoint count applied updates only. A skipped
    accumulating update still discards `accum`, as zero_grad() after a skipped scaler step does; BN
    running statistics of the bad batch's forward are not rolled back (nor does torch). Every kind then
    runs f3_optim_step / f3_net_backward_optim with one flat update after the backward, plain RMSprop
    included. The setting is fixed for the life of the step (read-only). False (the default) issues
    exactly the launches the step always issued.

    `ema_decay` (torch.optim.swa_utils.AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay)), or
    timm's ModelEma; the reference's loop has no averaging): a number in [0, 1] keeps one averaged copy of the
    parameters in the flat `ema` (a copy of the parameters at construction, as AveragedModel deep-copies) and
    advances it with one launch pair (ema_update(): f3_ema_update) after every optimizer update, on the
    stream the update ran on: eager on all three routes, on the update calls of an accumulating step, and
    inside the optimizer graph of a captured one. The first update copies the parameters, every later one
    is ema + (1 - decay) (p - ema) in fp64, rounded once (include/fall3.h); BatchNorm buffers are not
    averaged (use_buffers=False). The count (`n_averaged`, a 1-element int64 device view) and the decay live
    in the device block `ema_state` and are read when the launch runs: a replay advances the count, and
    `step.ema_decay = d` (one eager launch, never inside a capture) is followed by the next replay. A
    skip_nonfinite skip does not suppress the EMA update: torch's loop calls ema.update_parameters(model)
    whether or not scaler.step applied, so the average moves toward the unchanged parameters and n_averaged
    advances. Data parallel: no collective, every rank averages identical parameters with a deterministic
    kernel. The average is used through ema_state_dict() (model.state_dict() with the averaged parameters),
    `with step.swap_ema():` (the model holds the averaged weights inside it, same pointers), and
    ema_checkpoint() / load_ema_checkpoint(). None (the default): no buffer, no block, no launch."""

    def __init__(self, model, batch, lr=1e-3, alpha=0.99, eps=1e-8, process_group=None, optimizer=None,
                 phased=None, force_sync=False, max_norm=None, metrics=None, label_smoothing=0.0, accum_iter=1,
                 ema_decay=None, class_weight=None, skip_nonfinite=False):
        if not isinstance(skip_nonfinite, bool):
            raise ValueError(f"TrainStep: skip_nonfinite must be True or False, got {skip_nonfinite!r}")
        self._skip_nonfinite = skip_nonfinite
        self._ema_decay = None if ema_decay is None else check_ema_decay(ema_decay)
        self.label_smoothing, self.accum_iter = check_step_args(label_smoothing, accum_iter)
        if self.accum_iter > 1 and phased:
            raise ValueError("TrainStep: an accumulating step runs the whole backward per micro-batch (phased=True "
                             "overlaps an all-reduce that only update calls issue)")
        self.model = model
        self.N = batch
        self.lr, self.alpha, self.eps = lr, alpha, eps
        self.optimizer = optimizer
        self.max_norm = max_norm
        self.kind = _optim.optimizer_kind(optimizer) if optimizer is not None else "rmsprop"
        dev = model.flat_parameters().device
        nat = model._native
        self.grads = torch.zeros(nat.nparam, dtype=torch.float32, device=dev)
        # flat optimizer states, per kind (state0 / state1 of f3_optim_step)
        group = self._group()
        _optim.check_supported(self.kind, group)
        self._state = {k: torch.zeros(nat.nparam, dtype=torch.float32, device=dev)
                       for k in _optim.state_keys(self.kind, group)}
        self.square_avg = self._state.get("square_avg")
        self.momentum_buffer = self._state.get("momentum_buffer")
        self.exp_avg, self.exp_avg_sq = self._state.get("exp_avg"), self._state.get("exp_avg_sq")
        # step scalars (f3_optim_scalars_bytes): device step count, bias corrections, clip coefficient, norm
        self.scalars = ops.optim_scalars(dev)
        self.step_count, _, _, self.clip_coef, self.grad_norm = ops.scalar_views(self.scalars)
        # the guard words (skip_nonfinite): updates skipped so far, and whether the last one was
        self.skipped, self.last_skipped = ops.guard_views(self.scalars)
        self._legacy_steps = 0  # steps of the plain-RMSprop launches (which keep no device count)
        self._graph_legacy = False
        # a captured step's hyper-parameter block (f3_optim_hyper_bytes), the structure its optimizer graph
        # was recorded for and the values last written to the block; capture() sets all three
        self.hyper = None
        self._hyper_key = self._hyper_values = None
        # the entries no backward writes (f3_net_entry_nograd): skipped by every non-RMSprop update
        h0 = nat.h
        self._nograd = {name for i, (name, kind, _, _) in enumerate(nat.entries)
                        if kind == ENTRY_PARAM and lib().f3_net_entry_nograd(h0, i) == 1}
        self._skip = []
        for name, shape, off in model.param_views():
            if name in self._nograd:
                n4 = (int(np.prod(shape)) + 3) // 4 * 4
                if self._skip and self._skip[-2] + self._skip[-1] == off:
                    self._skip[-1] += n4
                else:
                    self._skip += [off, n4]
        self.ws = torch.empty(nat.workspace_bytes(batch), dtype=torch.uint8, device=dev)
        self.out = torch.empty(batch, model.spec.num_class, dtype=torch.float32, device=dev)
        self.dout = torch.empty_like(self.out)
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)
        # the class weights (class_weight): a device f32[C] tensor the loss launch reads when it runs
        self._class_weight = None
        if class_weight is not None:
            self._class_weight = torch.from_numpy(check_class_weight(class_weight, model.spec.num_class)).to(dev)
        if metrics is True:
            metrics = _metrics.StepMetrics(model.spec.num_class, top_k=(1,), device=dev)
        if metrics is not None and (not isinstance(metrics, _metrics.StepMetrics)
                                    or metrics.num_class != model.spec.num_class or metrics.device != dev):
            raise ValueError(f"TrainStep: metrics must be a StepMetrics for {model.spec.num_class} classes on {dev}")
        self.metrics = metrics
        self._grad_norms = None
        self.pg = process_group
        h = nat.h
        # accumulation (accum_iter > 1): the flat accumulator, the device word that makes the next
        # micro-batch overwrite it (set = model.zero_grad() has run), the position in the epoch
        self.accum = None
        self.pending = 0
        self._i, self._num_batches = 0, None
        if self.accum_iter > 1:
            self.accum = torch.zeros(nat.nparam, dtype=torch.float32, device=dev)
            self._accum_reset = torch.ones(1, dtype=torch.int32, device=dev)
        # the gradient the update, the all-reduce and the reports consume
        self._gsrc = self.grads if self.accum is None else self.accum
        if self.accum is None:
            self.sync = GradSync(self.grads, lib().f3_net_grad_split(h), process_group,
                                 wait_phase1=lambda st: check(lib().f3_net_wait_phase1(h, st), "wait phase 1"),
                                 force=force_sync)
        else:
            # issued after the accumulate launch on the caller's stream, on update calls only (the other
            # calls issue no collective: the saving of DDP's no_sync); not overlapped with the backward
            self.sync = GradSync(self.accum, lib().f3_net_grad_split(h), process_group, force=force_sync)
        self.world = self.sync.world
        # phased=True runs the two-phase backward even on one rank (times its cost against phase 0);
        # force_sync=True (tests) also issues the two all-reduce buckets at world 1
        self.phased = (self.world > 1 or force_sync) if phased is None else bool(phased)
        if self.accum is not None:
            self.phased = False
        # expose the flat gradient through the usual .grad attributes
        grad_views(model, self._gsrc)
        self.graph = None
        self._static = None
        # world 1: the RMSprop update per layer inside the backward (F3_FUSED_OPT=0: one launch after it)
        self.fused_optimizer = (not self.sync.active and self.accum is None
                                and os.environ.get("F3_FUSED_OPT", "1") != "0")
        # the parameter average (ema_decay): the flat copy, its device block (f3_ema_state_bytes: the count
        # and the decay, read by every update when it runs) and whether swap_ema() holds the model's weights
        self.ema = self.ema_state = self.n_averaged = None
        self._ema_swapped = False
        if self._ema_decay is not None:
            self.ema = model.flat_parameters().detach().clone()
            self.ema_state = ops.ema_state(dev)
            self.n_averaged, _ = ops.ema_views(self.ema_state)
            self._ema_write(self._ema_decay)

    # -- the pieces ------------------------------------------------------------
    def prepare(self, skel, sensor, label):
        """Validate a batch against the step's preallocated buffers (batch N, contiguous fp32 on the
        device) and turn 1-D class-index labels into one-hot targets as model/main.py:104-109 does."""
        m = self.model
        m.check_inputs(skel, sensor)
        for t, what in ((skel, "skel"), (sensor, "sensor")):
            if t is None:
                continue
            if t.shape[0] != self.N:
                raise ValueError(f"TrainStep was built for batch {self.N}, got {what} with batch {t.shape[0]}")
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"TrainStep: {what} must be contiguous fp32")
        dev = m.flat_parameters().device
        if label.dim() == 1:
            label = torch.nn.functional.one_hot(label.to(dev).long(), num_classes=m.spec.num_class).float()
        if tuple(label.shape) != (self.N, m.spec.num_class):
            raise ValueError(f"TrainStep: label must be [{self.N},{m.spec.num_class}] (or [{self.N}] class indices), "
                             f"got {tuple(label.shape)}")
        if label.device != dev or label.dtype != torch.float32 or not label.is_contiguous():
            label = label.to(device=dev, dtype=torch.float32).contiguous()
        return label

    def forward_loss(self, skel, sensor, label):
        L = lib()
        st = stream_handle()
        m = self.model
        m.native_forward(skel, sensor, self.out, self.ws, True, st)
        if self._class_weight is not None:
            check(L.f3_net_loss_w(m._native.h, self.N, ptr(self.out), ptr(label), ptr(self._class_weight),
                                  self.label_smoothing, ptr(self.loss), ptr(self.dout), st), "fall3 weighted loss")
        elif self.label_smoothing > 0.0:
            check(L.f3_net_loss_ex(m._native.h, self.N, ptr(self.out), ptr(label), self.label_smoothing,
                                   ptr(self.loss), ptr(self.dout), st), "fall3 smoothed loss")
        else:
            check(L.f3_net_loss(m._native.h, self.N, ptr(self.out), ptr(label), ptr(self.loss), ptr(self.dout), st),
                  "fall3 loss")
        if self.metrics is not None:
            self.metrics.update(self.out, label, self.loss)

    def backward_phase(self, phase):
        m = self.model
        check(lib().f3_net_backward_phase(m._native.h, self.N, ptr(m.flat_parameters()), ptr(self.dout),
                                          ptr(self.grads), ptr(self.ws), phase, stream_handle()),
              f"fall3 backward phase {phase}")

    def forward_backward(self, skel, sensor, label):
        self.forward_loss(skel, sensor, label)
        self.backward_phase(0)

    # -- optimizer plumbing ------------------------------------------------------
    def _group(self):
        """The hyper-parameters in force: the optimizer's param_groups[0], or the constructor's RMSprop values."""
        if self.optimizer is not None:
            return self.optimizer.param_groups[0]
        return {"lr": self.lr, "alpha": self.alpha, "eps": self.eps}

    @property
    def skip_nonfinite(self):
        """Whether the step skips an update on a non-finite gradient: fixed at construction."""
        return self._skip_nonfinite

    @property
    def class_weight(self):
        """A copy of the class weights in force (None: the step's loss is unweighted). Setting them validates
        the value (check_class_weight) and copies it into the device tensor in place, eagerly: the next step
        follows it, replayed ones included."""
        return None if self._class_weight is None else self._class_weight.clone()

    @class_weight.setter
    def class_weight(self, value):
        if self._class_weight is None or value is None:
            raise ValueError("TrainStep: class_weight can be changed only on a step built with class weights, and "
                             "not to None (the step, and a captured graph, hold another loss launch)")
        w = check_class_weight(value, self.model.spec.num_class)
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("TrainStep: the class weights are written eagerly, never inside a capture")
        self._class_weight.copy_(torch.from_numpy(w))

    def _legacy(self, group):
        """Plain RMSprop (no decay, no clipping, no guard): the launches of f3_rmsprop_step /
        f3_net_backward_rmsprop."""
        return (self.kind == "rmsprop" and not group.get("weight_decay", 0) and not self.max_norm
                and not self._skip_nonfinite)

    def _config(self, group, grad_scale):
        _optim.check_supported(self.kind, group)
        keys = _optim.state_keys(self.kind, group)
        for k in keys:
            if k not in self._state:  # e.g. a momentum set after construction
                self._state[k] = torch.zeros_like(self.grads)
                setattr(self, k, self._state[k])
        cfg = ops.optim_config(max_norm=float(self.max_norm or 0.0), grad_scale=grad_scale, skip=self._skip,
                               skip_nonfinite=self._skip_nonfinite, **_optim.hyper(self.kind, group))
        st = [self._state[k] for k in keys] + [None, None]
        return cfg, st[0], st[1]

    def _count_legacy(self):
        if not torch.cuda.is_current_stream_capturing():
            self._legacy_steps += 1

    def optimizer_step(self):
        """The flat update on `grads`, or on `accum` in an accumulating step, which then also sets the
        reset word (the model.zero_grad() of model/main.py:132: the next micro-batch overwrites)."""
        g = self._group()
        if self.optimizer is not None:
            self.lr, self.alpha, self.eps = g["lr"], g.get("alpha", self.alpha), g.get("eps", self.eps)
        scale = 1.0 / self.world
        src = self._gsrc
        if not self._legacy(g):
            cfg, s0, s1 = self._config(g, scale)
            check(lib().f3_optim_step(cfg, ptr(self.model.flat_parameters()), ptr(s0), ptr(s1), ptr(src),
                                      src.numel(), ptr(self.scalars), stream_handle()), f"{self.kind} step")
        else:
            self._count_legacy()
            check(lib().f3_rmsprop_step(ptr(self.model.flat_parameters()), ptr(self.square_avg), ptr(src),
                                        src.numel(), self.lr, self.alpha, self.eps, scale, stream_handle()),
                  "rmsprop")
        if self.accum is not None:
            self._accum_reset.fill_(1)

    # -- the captured update: structure fixed when recorded, values from the device block ---------
    def _hyper_now(self):
        """(structure key, the values in ops.HYPER_FIELDS order) of the group, max_norm and 1/world in force."""
        g = self._group()
        if self.optimizer is not None:
            self.lr, self.alpha, self.eps = g["lr"], g.get("alpha", self.alpha), g.get("eps", self.eps)
        _optim.check_supported(self.kind, g)
        h = _optim.hyper(self.kind, g)
        if self._legacy(g):  # the three values the eager plain-RMSprop launch passes
            h.update(lr=float(self.lr), alpha=float(self.alpha), eps=float(self.eps))
        h.update(max_norm=float(self.max_norm or 0.0), grad_scale=1.0 / self.world)
        return _optim.hyper_structure(self.kind, g, self.max_norm), tuple(h[k] for k in ops.HYPER_FIELDS)

    def _hyper_write(self, values):
        """One eager launch on the current stream (f3_optim_hyper_set), ordered before the next replay."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("TrainStep: the hyper-parameter block is written eagerly, never inside a capture")
        cfg = ops.optim_config(kind=_optim.KIND_IDS[self.kind], nesterov=False, **dict(zip(ops.HYPER_FIELDS, values)))
        check(lib().f3_optim_hyper_set(cfg, ptr(self.hyper), stream_handle()), f"{self.kind} hyper-parameters")
        self._hyper_values = values

    def _hyper_sync(self):
        """Before a replay of the optimizer graph: a changed structure raises (the graph holds other
        launches), changed values are written to the block, and nothing changed issues no launch."""
        key, values = self._hyper_now()
        if key != self._hyper_key:
            changed = [name for name, a, b in zip(_optim.STRUCTURE_FIELDS, self._hyper_key, key) if a != b]
            raise ValueError(f"TrainStep: {', '.join(changed)} changed since capture() ({self._hyper_key} -> {key}): "
                             "the captured optimizer graph runs other launches, capture the step again")
        if values != self._hyper_values:
            self._hyper_write(values)

    # -- the parameter average (ema_decay) -----------------------------------------------
    def _need_ema(self, what):
        if self.ema is None:
            raise ValueError(f"TrainStep.{what} needs ema_decay (this step keeps no parameter average)")

    def _ema_write(self, decay):
        """One eager launch on the current stream (f3_ema_set_decay), ordered before the next update or replay."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("TrainStep: the EMA decay is written eagerly, never inside a capture")
        check(lib().f3_ema_set_decay(ptr(self.ema_state), decay, stream_handle()), "ema decay")
        self._ema_decay = decay

    @property
    def ema_decay(self):
        """The decay in force (None: the step keeps no average). Setting it validates the value and writes
        it to the device block with one eager launch: the next update follows it, replayed ones included."""
        return self._ema_decay

    @ema_decay.setter
    def ema_decay(self, value):
        self._need_ema("ema_decay")
        self._ema_write(check_ema_decay(value))

    def ema_update(self):
        """ema_model.update_parameters(model): the one launch pair (f3_ema_update) on the current stream, the
        lerp over the flat parameters and then n_averaged += 1. The step issues it after every optimizer update."""
        self._need_ema("ema_update()")
        flat = self.model.flat_parameters()
        check(lib().f3_ema_update(ptr(self.ema), ptr(flat), flat.numel(), ptr(self.ema_state), stream_handle()),
              "ema update")

    def ema_state_dict(self):
        """model.state_dict() (keys, order, shapes) with the parameters taken from `ema`, as copies; the
        buffers are the model's current ones (use_buffers=False keeps them in sync with the model). Loads
        into the reference's module, and as {"model_weight": ...} through evaluate.load_best."""
        self._need_ema("ema_state_dict()")
        if self._ema_swapped:
            raise RuntimeError("TrainStep.ema_state_dict() inside swap_ema(): `ema` holds the raw weights there")
        views = {name: (shape, off) for name, shape, off in self.model.param_views()}
        sd = self.model.state_dict()
        out = type(sd)()
        for k, v in sd.items():
            if k in views:
                shape, off = views[k]
                out[k] = self.ema[off:off + int(np.prod(shape))].view(tuple(shape)).clone()
            else:
                out[k] = v.detach().clone()
        return out

    @contextlib.contextmanager
    def swap_ema(self):
        """Exchange the contents of model.flat_parameters() and `ema` in place, and exchange them back on
        exit, also when the body raises. Pointers do not change, so captured graphs and the p.grad views
        stay valid; evaluate.valid_device(model, loader) / test_device inside it evaluate the averaged
        weights unchanged. Calling the step inside the context raises RuntimeError."""
        self._need_ema("swap_ema()")
        if self._ema_swapped:
            raise RuntimeError("TrainStep.swap_ema() does not nest")
        self._ema_exchange()
        self._ema_swapped = True
        try:
            yield self.model
        finally:
            self._ema_exchange()
            self._ema_swapped = False

    def _ema_exchange(self):
        flat = self.model.flat_parameters()
        with torch.no_grad():
            held = flat.detach().clone()
            flat.copy_(self.ema)
            self.ema.copy_(held)

    def ema_checkpoint(self):
        """{"n_averaged": int, "decay": float, "params": {name: cpu tensor}} in model.named_parameters() order
        (reads the device count: a host sync)."""
        self._need_ema("ema_checkpoint()")
        if self._ema_swapped:
            raise RuntimeError("TrainStep.ema_checkpoint() inside swap_ema(): `ema` holds the raw weights there")
        views = {name: (shape, off) for name, shape, off in self.model.param_views()}
        params = {}
        for n, _ in self.model.named_parameters():
            shape, off = views[n]
            params[n] = self.ema[off:off + int(np.prod(shape))].view(tuple(shape)).cpu().clone()
        return {"n_averaged": int(self.n_averaged.item()), "decay": float(self._ema_decay), "params": params}

    def load_ema_checkpoint(self, d):
        """Restore the average, the count and the decay from ema_checkpoint()'s dict, in place: a captured
        graph stays valid, and its next replay continues from the loaded state."""
        self._need_ema("load_ema_checkpoint()")
        if self._ema_swapped:
            raise RuntimeError("TrainStep.load_ema_checkpoint() inside swap_ema()")
        decay = check_ema_decay(d["decay"])
        n_averaged = int(d["n_averaged"])
        views = {name: (shape, off) for name, shape, off in self.model.param_views()}
        names = [n for n, _ in self.model.named_parameters()]
        missing = [n for n in names if n not in d["params"]]
        if n_averaged < 0 or missing:
            raise ValueError(f"TrainStep.load_ema_checkpoint: n_averaged {n_averaged}, missing parameters {missing}")
        for n in names:
            shape, off = views[n]
            t = d["params"][n]
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"TrainStep.load_ema_checkpoint: {n} has shape {tuple(t.shape)}, not {tuple(shape)}")
        for n in names:
            shape, off = views[n]
            self.ema[off:off + int(np.prod(shape))].view(tuple(shape)).copy_(d["params"][n])
        self.n_averaged.fill_(n_averaged)
        self._ema_write(decay)

    # -- accumulation (accum_iter > 1) ----------------------------------------------
    def _need_accum(self, what):
        if self.accum is None:
            raise ValueError(f"TrainStep.{what} needs accum_iter > 1 (this step updates on every call)")

    def accumulate(self):
        """accum = grads (after an update or zero_grad()) or accum + grads: one launch, then the reset
        word is cleared on the stream."""
        self._need_accum("accumulate()")
        check(lib().f3_grad_accumulate(ptr(self.accum), ptr(self.grads), self.grads.numel(),
                                       ptr(self._accum_reset), stream_handle()), "fall3 grad accumulate")

    def begin_epoch(self, num_batches):
        """Start counting batches at 0 for the reference's update rule (accum_updates): the epoch's
        last batch then updates too. Without it the count runs on and nothing is flushed at an epoch's end."""
        self._i, self._num_batches = 0, int(num_batches)

    def zero_grad(self):
        """Discard a pending accumulation: the next micro-batch overwrites `accum`."""
        self._need_accum("zero_grad()")
        self._accum_reset.fill_(1)
        self.pending = 0

    def _update_due(self, update):
        i = self._i
        self._i += 1
        if update is not None:
            return bool(update)
        return i % self.accum_iter == 0 or (self._num_batches is not None and i + 1 == self._num_batches)

    def backward_optimizer_step(self):
        """loss.backward() + optimizer.step() in one native call (world 1): each skeleton layer's
        RMSprop update starts on the queue that finishes its gradients (f3_net_backward_rmsprop);
        self.grads holds the gradients afterwards as with backward_phase(0)."""
        g = self._group()
        if self.optimizer is not None:
            self.lr, self.alpha, self.eps = g["lr"], g.get("alpha", self.alpha), g.get("eps", self.eps)
        m = self.model
        if not self._legacy(g):
            # the generalisation (f3_net_backward_optim): per-layer updates of any kind, or with clipping
            # one flat update after the join (the norm needs every gradient)
            cfg, s0, s1 = self._config(g, 1.0)
            check(lib().f3_net_backward_optim(m._native.h, self.N, ptr(m.flat_parameters()), ptr(self.dout),
                                              ptr(self.grads), ptr(s0), ptr(s1), ptr(self.scalars), ptr(self.ws),
                                              cfg, stream_handle()), f"fall3 backward + {self.kind}")
            return
        self._count_legacy()
        check(lib().f3_net_backward_rmsprop(m._native.h, self.N, ptr(m.flat_parameters()), ptr(self.dout),
                                            ptr(self.grads), ptr(self.square_avg), ptr(self.ws), self.lr, self.alpha,
                                            self.eps, stream_handle()), "fall3 backward + rmsprop")

    def allreduce(self):
        self.sync.all()

    # -- one step ----------------------------------------------------------------
    def _eager(self, skel, sensor, label):
        self.forward_loss(skel, sensor, label)
        if self.phased:
            self.backward_phase(1)
            self.sync.start_head()       # after phase 1's queues, concurrent with phase 2
            self.backward_phase(2)
            self.sync.start_tail()
            self.sync.finish()
        elif self.fused_optimizer:
            self.backward_optimizer_step()
            if self.ema is not None:
                self.ema_update()
            return
        else:
            self.backward_phase(0)
        self.optimizer_step()
        if self.ema is not None:
            self.ema_update()

    def _accum_call(self, skel, sensor, label, update):
        """One micro-batch of an accumulating step; the all-reduce and the update on update calls only."""
        do_update = self._update_due(update)
        if do_update and self.graph is not None:
            self._hyper_sync()  # raises before anything runs; a write is ordered before the replay below
        if self.graph is None:
            self.forward_backward(skel, sensor, label)
            self.accumulate()
        else:
            self._load_static(skel, sensor, label)
            self.graph[0].replay()
        self.pending += 1
        if do_update:
            self.sync.all()
            if self.graph is None:
                self.optimizer_step()
                if self.ema is not None:
                    self.ema_update()
            else:
                if self._graph_legacy:
                    self._legacy_steps += 1
                self.graph[2].replay()
            self.pending = 0
        return self.loss

    def _load_static(self, skel, sensor, label):
        s = self._static
        if skel is not None and skel.data_ptr() != s[0].data_ptr():
            s[0].copy_(skel)
        if sensor is not None and sensor.data_ptr() != s[1].data_ptr():
            s[1].copy_(sensor)
        if label.data_ptr() != s[2].data_ptr():
            s[2].copy_(label)

    def __call__(self, skel, sensor, label, update=None):
        """One batch. `update` (accumulating steps only): True / False decides whether this call ends
        with the optimizer update, instead of the reference's rule counted from begin_epoch()."""
        if self._ema_swapped:
            raise RuntimeError("TrainStep: called inside swap_ema(): the model holds the averaged weights, a step "
                               "would train them")
        label = self.prepare(skel, sensor, label)
        if self.accum is not None:
            return self._accum_call(skel, sensor, label, update)
        if update is not None and not update:
            self._need_accum("__call__(update=False)")
        if self.graph is None:
            self._eager(skel, sensor, label)
            return self.loss
        self._hyper_sync()  # raises before anything runs; a write is ordered before g_opt's replay
        self._load_static(skel, sensor, label)
        g_head, g_tail, g_opt = self.graph
        if self._graph_legacy:
            self._legacy_steps += 1
        g_head.replay()
        if g_tail is not None:
            # the captured phase 1 joined its queues into the capturing stream (net.cpp
            # mark_phase1), so the head bucket is ordered after the replay itself
            self.sync.start_head(after_current=True)  # RCCL on the comm stream, concurrent with phase 2
            g_tail.replay()
            self.sync.start_tail()
            self.sync.finish()
        g_opt.replay()
        return self.loss

    def capture(self, skel, sensor, label, warmup=2):
        """Capture the step into HIP graphs; the given tensors become the static inputs
        (later calls copy new batches into them). world == 1: [fwd+loss+bwd], [RMSprop].
        world > 1: [fwd+loss+bwd phase 1], [bwd phase 2], [RMSprop], with the two all-reduce
        buckets issued between replays. accum_iter > 1: [fwd+loss+bwd+accumulate], [update on
        accum, set the reset word]; the second is replayed on update calls only, after the all-reduce
        of accum at world > 1. A pending accumulation is kept. The optimizer graph holds
        f3_optim_step_hyper: the hyper-parameters in force are written to the device block here and
        whenever they have changed before a replay, so the captured step follows a scheduler."""
        self._static = (skel, sensor, label)
        kept = self.metrics.snapshot() if self.metrics is not None else None  # the warm-up steps must not count
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self.forward_backward(skel, sensor, label)
        torch.cuda.current_stream().wait_stream(side)
        if kept is not None:
            self.metrics.restore(kept)
        torch.cuda.synchronize()
        g_head = torch.cuda.CUDAGraph()
        g_tail = None
        if self.phased:
            with torch.cuda.graph(g_head):
                self.forward_loss(skel, sensor, label)
                self.backward_phase(1)
            g_tail = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g_tail):
                self.backward_phase(2)
        elif self.accum is not None:
            # the micro-step in its one form: the accumulate launch reads the reset word when replayed;
            # the optimizer graph below reads accum and ends by setting the word
            with torch.cuda.graph(g_head):
                self.forward_backward(skel, sensor, label)
                self.accumulate()
        else:
            with torch.cuda.graph(g_head):
                self.forward_backward(skel, sensor, label)
        # the update in its device-reading form (f3_optim_step_hyper): the graph fixes which launches run
        # (the structure key), the block written here and before later replays (_hyper_sync) gives the values
        key, values = self._hyper_now()
        cfg, s0, s1 = self._config(self._group(), 1.0 / self.world)
        if self.hyper is None:
            self.hyper = ops.optim_hyper(self.grads.device)
        self._hyper_write(values)
        src = self._gsrc
        g_opt = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_opt):
            check(lib().f3_optim_step_hyper(cfg, ptr(self.model.flat_parameters()), ptr(s0), ptr(s1), ptr(src),
                                            src.numel(), ptr(self.hyper), ptr(self.scalars), stream_handle()),
                  f"{self.kind} step")
            if self.ema is not None:
                self.ema_update()  # reads the count and the decay on replay
            if self.accum is not None:
                self._accum_reset.fill_(1)
        self._hyper_key = key
        self._graph_legacy = self._legacy(self._group())
        self.graph = (g_head, g_tail, g_opt)

    # -- reporting -----------------------------------------------------------------
    def param_grad_norms(self):
        """(names, norms): names in model.named_parameters() order; norms a device fp32 tensor of
        len(names) + 1 values, the L2 norm of each parameter's gradient and then of all of them, of the
        gradient the last update consumed (self.grads, or self.accum in an accumulating step, times
        1/world; between updates `accum` holds the sum so far). Two launches, no sync (the
        reference's visualize_weights_and_gradients calls .item() per parameter, model/main.py:84-89).
        The same tensor is returned by every call: clone it to keep a step's values."""
        if self._grad_norms is None:
            views = {name: (shape, off) for name, shape, off in self.model.param_views()}
            names = [n for n, _ in self.model.named_parameters()]
            self._grad_norms = (names, _metrics.SegmentNorms(self._gsrc, [views[n][1] for n in names],
                                                             [int(np.prod(views[n][0])) for n in names]))
        names, seg = self._grad_norms
        return list(names), seg(1.0 / self.world)

    # -- checkpoint (model/main.py:302 optimizer.load_state_dict, :336 "optimizer": optimizer.state_dict()) --
    def _layout(self):
        """[(shape, flat offset, nograd)] in model.parameters() order."""
        views = {name: (shape, off) for name, shape, off in self.model.param_views()}
        return [(tuple(views[n][0]), views[n][1], n in self._nograd) for n, _ in self.model.named_parameters()]

    def steps_taken(self):
        """Optimizer steps so far (reads the device count: a host sync)."""
        return int(self.step_count.item()) + self._legacy_steps

    def skipped_steps(self):
        """Updates skipped for a non-finite gradient so far (skip_nonfinite; reads the device count: a host
        sync). steps_taken() and the checkpoint's `step` count the applied ones only."""
        return int(self.skipped.item())

    def optimizer_state_dict(self):
        """torch.optim.<kind>(model.parameters()).state_dict() of this step's optimizer state: loads into
        torch's optimizer, into f3's, and back into a TrainStep (load_optimizer_state_dict). `step` counts
        updates, not micro-batches; a pending accumulation is not saved (the reference checkpoints at
        epoch ends, model/main.py:336, where nothing is pending)."""
        group = self._group()
        full = _optim.torch_defaults(self.kind)
        full.update({k: v for k, v in group.items() if k != "params"})
        keys = _optim.state_keys(self.kind, full)
        return _optim.flat_to_state_dict(self.kind, full, self._layout(), [self._state[k] for k in keys],
                                         self.steps_taken())

    def load_optimizer_state_dict(self, sd):
        """Restore the flat states, the step count and the hyper-parameters from a state_dict written by
        optimizer_state_dict() or by torch.optim.<kind>(model.parameters()) (in place: a captured graph stays valid,
        and its next replay runs with the loaded hyper-parameters)."""
        bufs, step, group = _optim.state_dict_to_flat(self.kind, sd, self._layout(), self.grads.numel(),
                                                      device=self.grads.device)
        keys = _optim.state_keys(self.kind, group)
        for k, b in zip(keys, bufs):
            if k not in self._state:
                self._state[k] = torch.zeros_like(self.grads)
                setattr(self, k, self._state[k])
            self._state[k].copy_(b)
        self.step_count.fill_(step)
        self._legacy_steps = 0
        hyper = {k: v for k, v in group.items() if k != "params"}
        if self.optimizer is not None:
            self.optimizer.param_groups[0].update(hyper)
        else:
            self.lr, self.alpha, self.eps = hyper.get("lr", self.lr), hyper.get("alpha", self.alpha), hyper.get(
                "eps", self.eps)
