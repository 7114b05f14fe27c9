"""Step metrics kept on the device: what the reference's loop reports per batch and per epoch,
without a device-to-host copy or a stream sync per batch.

  running loss, top-k accuracy per batch    model/main.py:57-77 (cal_top_k_accuracy), 134-135
  confusion matrix, macro P/R/F1            model/main.py:189-200, 230-245, main_cross_validation.py:247

`StepMetrics.update` is one launch of f3_metrics_update (include/fall3.h) on the current stream; it
can be captured into a HIP graph (TrainStep(metrics=...) does so). `result()` makes the one copy to
the host; `summarize` is numpy only and needs neither sklearn nor a device.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ._lib import METRICS_MAXC, METRICS_MAXK, check, lib, ptr, require_device, stream_handle

_HEAD = 2 + METRICS_MAXK  # int64 words between loss_sum and the confusion matrix


def check_args(num_class, top_k):
    """The constructor's checks (no device needed): 1 <= num_class <= 64, 1 <= k <= num_class, at most 8 k."""
    num_class = int(num_class)
    if not 1 <= num_class <= METRICS_MAXC:
        raise ValueError(f"StepMetrics: num_class must be in 1..{METRICS_MAXC} (the confusion tile is held in LDS), "
                         f"got {num_class}")
    top_k = tuple(int(k) for k in top_k)
    if len(top_k) > METRICS_MAXK:
        raise ValueError(f"StepMetrics: at most {METRICS_MAXK} top_k entries, got {len(top_k)}")
    for k in top_k:
        if not 1 <= k <= num_class:
            raise ValueError(f"StepMetrics: top_k entry {k} outside 1..num_class={num_class}")
    return num_class, top_k


def check_batch(out, label, loss, num_class, device=None):
    """update()'s checks: `out` contiguous fp32 [N, num_class], `label` int64 [N] or contiguous fp32
    [N, num_class], `loss` (optional) a 1-element fp32 tensor, all on the (same) HIP device. Returns N."""
    for t, what in ((out, "out"), (label, "label")) + (((loss, "loss"),) if loss is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"StepMetrics.update: {what} must be a tensor")
        require_device(t, f"StepMetrics.update: {what}")
        if device is not None and t.device != device:
            raise ValueError(f"StepMetrics.update: {what} is on {t.device}, the accumulators on {device}")
        if not t.is_contiguous():
            raise ValueError(f"StepMetrics.update: {what} must be contiguous")
    if out.dim() != 2 or out.shape[1] != num_class or out.shape[0] < 1 or out.dtype != torch.float32:
        raise ValueError(f"StepMetrics.update: out must be fp32 [N,{num_class}] with N >= 1, got {out.dtype} "
                         f"{tuple(out.shape)}")
    N = out.shape[0]
    if label.dim() == 1:
        if label.dtype != torch.int64 or label.shape[0] != N:
            raise ValueError(f"StepMetrics.update: a 1-D label must be int64 [{N}], got {label.dtype} "
                             f"{tuple(label.shape)}")
    elif label.dim() != 2 or tuple(label.shape) != (N, num_class) or label.dtype != torch.float32:
        raise ValueError(f"StepMetrics.update: label must be int64 [{N}] or fp32 [{N},{num_class}], got "
                         f"{label.dtype} {tuple(label.shape)}")
    if loss is not None and (loss.dtype != torch.float32 or loss.numel() != 1):
        raise ValueError("StepMetrics.update: loss must be a 1-element fp32 tensor")
    return N


def summarize(loss_sum, batches, rows, correct, confusion, top_k):
    """The epoch's figures from the accumulated block (numpy, fp64):
      loss         mean of the per-batch mean losses (None before the first update)
      top_k        correct[j] / rows per requested k (None entries before the first row)
      confusion    [C][C] counts, row = true class, column = predicted class
      precision, recall, f1   macro averages as precision_recall_fscore_support(average="macro",
                   zero_division=0) without labels= gives them (evaluate.class_metrics): over the
                   classes that occur among the true or the predicted labels; a zero denominator gives 0
      specificity  per class TN / (TN + FP), 0 where the denominator is 0
      batches, rows"""
    cm = np.asarray(confusion, dtype=np.int64)
    if cm.ndim != 2 or cm.shape[0] != cm.shape[1]:
        raise ValueError(f"summarize: confusion must be square, got {cm.shape}")
    batches, rows = int(batches), int(rows)
    correct = [int(c) for c in np.asarray(correct).reshape(-1)[:len(top_k)]]
    tp = np.diag(cm)
    true_sum, pred_sum = cm.sum(1), cm.sum(0)
    fp, fn = pred_sum - tp, true_sum - tp
    tn = cm.sum() - tp - fp - fn

    def ratio(num, den):
        return np.where(den > 0, num / np.maximum(den, 1), 0.0)

    present = (true_sum + pred_sum) > 0
    prec, rec, f1 = ratio(tp, pred_sum), ratio(tp, true_sum), ratio(2 * tp, true_sum + pred_sum)

    def macro(v):
        return float(np.mean(v[present])) if present.any() else 0.0

    return {"loss": float(loss_sum) / batches if batches else None,
            "top_k": [c / rows if rows else None for c in correct],
            "confusion": cm.tolist(),
            "precision": macro(prec), "recall": macro(rec), "f1": macro(f1),
            "specificity": ratio(tn, tn + fp).tolist(),
            "batches": batches, "rows": rows}


class StepMetrics:
    """Loss, top-k and confusion accumulators in one device block (layout: include/fall3.h).

    `loss_sum` (fp64[1]) and `counts` (int64: batches, rows, correct[8], confusion[C*C]) are views of
    the block, so a data-parallel caller can all-reduce them itself before `result()`."""

    def __init__(self, num_class, top_k=(1, 5), device=None):
        self.num_class, self.top_k = check_args(num_class, top_k)
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise RuntimeError("fall3: StepMetrics accumulates on the HIP device (MI355X); there is no CPU path")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        nbytes = int(lib().f3_metrics_bytes(self.num_class))
        self.block = torch.zeros(nbytes // 8, dtype=torch.int64, device=dev)
        self.loss_sum = self.block[0:1].view(torch.float64)
        self.counts = self.block[1:]
        self._k = (ctypes.c_int * max(len(self.top_k), 1))(*self.top_k)

    def reset(self):
        check(lib().f3_metrics_reset(ptr(self.block), self.num_class, stream_handle(self.device)), "metrics reset")

    def update(self, out, label, loss=None):
        """Add one batch (one launch on the current stream, no sync). A 1-D int64 label holds class
        indices, a 2-D fp32 label soft or one-hot targets. loss=None: the soft-target CE of `out` is
        computed by the kernel; otherwise the 1-element device tensor a loss launch wrote is added."""
        N = check_batch(out, label, loss, self.num_class, self.device)
        soft, idx = (label, None) if label.dim() == 2 else (None, label)
        check(lib().f3_metrics_update(ptr(self.block), ptr(out), ptr(soft), ptr(idx), ptr(loss), N, self.num_class,
                                      self._k, len(self.top_k), stream_handle(self.device)), "metrics update")

    def snapshot(self):
        """A copy of the block on the device (restore() puts it back): TrainStep.capture() keeps its
        warm-up and capture launches from counting with these."""
        return self.block.clone()

    def restore(self, snap):
        self.block.copy_(snap)

    def result(self):
        """One device-to-host copy of the block, then summarize()."""
        blk = self.block.cpu().numpy()
        C = self.num_class
        return summarize(blk[0:1].view(np.float64)[0], blk[1], blk[2], blk[3:3 + len(self.top_k)],
                         blk[1 + _HEAD:].reshape(C, C), self.top_k)


class SegmentNorms:
    """L2 norms of fixed segments of one flat fp32 buffer plus the norm of all of them together
    (f3_segment_norms): the table and the scratch are built once, each call is two launches, no sync."""

    def __init__(self, flat, offsets, lengths):
        require_device(flat, "SegmentNorms: the flat buffer")
        if flat.dtype != torch.float32 or not flat.is_contiguous() or flat.dim() != 1:
            raise ValueError("SegmentNorms: a contiguous 1-D fp32 buffer is required")
        offsets, lengths = [int(o) for o in offsets], [int(n) for n in lengths]
        if len(offsets) != len(lengths):
            raise ValueError("SegmentNorms: one length per offset")
        for o, n in zip(offsets, lengths):
            if o % 4 or o < 0 or n < 0 or o + n > flat.numel():
                raise ValueError(f"SegmentNorms: segment [{o}, {o + n}) must start at a multiple of 4 floats "
                                 f"inside the buffer of {flat.numel()}")
        self.flat, self.nseg = flat, len(offsets)
        dev = flat.device
        self.table = torch.tensor([offsets, lengths], dtype=torch.int64).reshape(2, -1).to(dev)
        self.scratch_bytes = int(lib().f3_segment_norms_scratch_bytes(sum(lengths), self.nseg))
        self.scratch = torch.zeros(self.scratch_bytes // 8, dtype=torch.float64, device=dev)
        self.norms = torch.zeros(self.nseg + 1, dtype=torch.float32, device=dev)

    def __call__(self, scale=1.0):
        """norms[s] = scale * ||segment s||, norms[nseg] = scale * ||all segments|| (the same device
        tensor every call: clone it to keep a step's values)."""
        check(lib().f3_segment_norms(ptr(self.flat), ptr(self.table[0]), ptr(self.table[1]), self.nseg,
                                     ptr(self.norms), ptr(self.scratch), self.scratch_bytes, float(scale),
                                     stream_handle(self.flat.device)), "segment norms")
        return self.norms
