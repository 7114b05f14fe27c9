"""What the four native-backed models share on the Python side of the C ABI.

  NativeHandle   owner of one f3_<prefix> handle: its state_dict table, its counts and its workspace size
  FlatModule     nn.Module whose parameters, buffers and counters are views into one flat array each,
                 registered under the reference's names in entry-table order; re-aliased after .to()
  _SideStep      fused forward -> soft-target CE -> backward -> RMSprop step of the three side models
                 (TargcnStep, SktrStep, MusaStep); TrainStep (train.py) stays on its own

A model class fills its config struct (a NativeHandle subclass), gives the initial value of every entry
(`_default`) and keeps its own input check, native_forward / native_backward and forward.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import ops
from ._lib import ENTRY_BUFFER, ENTRY_PARAM, check, lib, ptr, stream_handle


class NativeHandle:
    """Owner of one f3_<prefix> handle and its state_dict table: entries = [(name, kind, shape, offset)]."""

    def __init__(self, prefix, config):
        L = lib()
        self._prefix = prefix
        h = ctypes.c_void_p()
        check(self._fn("create")(ctypes.byref(config), ctypes.byref(h)), f"f3_{prefix}_create")
        self.h = h
        self.entries = []
        name, kind, nd = ctypes.c_char_p(), ctypes.c_int(), ctypes.c_int()
        shape, off = (ctypes.c_int64 * 8)(), ctypes.c_int64()
        for i in range(self._fn("num_entries")(h)):
            check(self._fn("entry")(h, i, ctypes.byref(name), ctypes.byref(kind), ctypes.byref(nd), shape,
                                    ctypes.byref(off)), f"f3_{prefix}_entry")
            self.entries.append((name.value.decode(), kind.value, tuple(shape[d] for d in range(nd.value)),
                                 off.value))
        self.nparam = self._fn("param_count")(h)
        self.nbuf = self._fn("buffer_count")(h)
        # f3_targcn has no counters and no f3_targcn_counter_count
        self.has_counters = hasattr(L, f"f3_{prefix}_counter_count")
        self.ncnt = self._fn("counter_count")(h) if self.has_counters else 0
        self._ws_bytes = {}

    def _fn(self, name):
        return getattr(lib(), f"f3_{self._prefix}_{name}")

    def workspace_bytes(self, batch):
        if batch not in self._ws_bytes:
            self._ws_bytes[batch] = int(self._fn("workspace_bytes")(self.h, batch))
        return self._ws_bytes[batch]

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self._fn("destroy")(self.h)
        except Exception:
            pass


def grad_views(model, grads, skip=lambda name: False):
    """Hang .grad views into the flat gradient array `grads` on the model's parameters (none where skip(name))."""
    for (name, shape, off), p in zip(model.param_views(), model.parameters()):
        if not skip(name):
            p.grad = grads[off:off + int(np.prod(shape))].view(shape)


class FlatModule(nn.Module):
    """Native-backed module over flat storage: `_flat_params` (fp32), `_flat_buffers` (fp32) and
    `_flat_counters` (int64; None where the native net has no counters). A subclass calls `_build` at the
    end of its constructor and provides `_default`; `_requires_grad` may freeze a parameter."""

    def _build(self, native, n_class, device):
        """Allocate the flat arrays on `device` and register every entry of the native table, in table
        order, as a view holding `_default(name, shape, shapes)` (shapes: name -> shape of every entry).
        The defaults draw from the global torch RNG, one call per entry in this order."""
        object.__setattr__(self, "_native", native)
        object.__setattr__(self, "_n_class", int(n_class))
        object.__setattr__(self, "_op_id", ops.register(self))
        if device is None:
            device = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
        self._alloc(torch.device(device))
        shapes = {n: s for n, k, s, o in native.entries}
        with torch.no_grad():
            for name, kind, shape, off in native.entries:
                t = self._view(kind, shape, off)
                t.copy_(self._default(name, shape, shapes))
                mod, leaf = self._owner(name)
                if kind == ENTRY_PARAM:
                    mod.register_parameter(leaf, nn.Parameter(t, requires_grad=self._requires_grad(name)))
                else:
                    mod.register_buffer(leaf, t)

    def _default(self, name, shape, shapes):
        raise NotImplementedError

    def _requires_grad(self, name):
        return True

    @property
    def n_class(self):
        """Width of the logits (the class count the native net was created with)."""
        return self._n_class

    @property
    def _counters(self):
        return self._flat_counters

    def _alloc(self, dev):
        nat = self._native
        object.__setattr__(self, "_flat_params", torch.zeros(nat.nparam, dtype=torch.float32, device=dev))
        object.__setattr__(self, "_flat_buffers", torch.zeros(max(nat.nbuf, 1), dtype=torch.float32, device=dev))
        object.__setattr__(self, "_flat_counters", torch.zeros(max(nat.ncnt, 1), dtype=torch.int64, device=dev)
                           if nat.has_counters else None)

    def _view(self, kind, shape, off):
        n = int(np.prod(shape)) if len(shape) else 1
        flat = (self._flat_params if kind == ENTRY_PARAM else
                self._flat_buffers if kind == ENTRY_BUFFER else self._flat_counters)
        return flat[off:off + n].view(shape)

    def _owner(self, name):
        mod = self
        *path, leaf = name.split(".")
        for p in path:
            if p not in mod._modules:
                mod.add_module(p, nn.Module())
            mod = mod._modules[p]
        return mod, leaf

    def _tensor(self, name):
        mod, leaf = self._owner(name)
        return mod._parameters[leaf] if leaf in mod._parameters else mod._buffers[leaf]

    def _apply(self, fn, recurse=True):
        """.to() / .cuda() / .float(): re-alias every tensor into fresh flat arrays on the new device. The
        Parameter objects keep their identity; storage stays fp32 / int64 whatever dtype was asked for."""
        super()._apply(fn, recurse)
        self._alloc(next(iter(self.parameters())).device)
        with torch.no_grad():
            for name, kind, shape, off in self._native.entries:
                cur = self._tensor(name)
                view = self._view(kind, shape, off)
                view.copy_(cur.detach())
                if kind == ENTRY_PARAM:
                    cur.data = view
                else:
                    mod, leaf = self._owner(name)
                    mod._buffers[leaf] = view
        return self

    def flat_parameters(self):
        return self._flat_params

    def param_views(self):
        return [(name, shape, off) for name, kind, shape, off in self._native.entries if kind == ENTRY_PARAM]


class _SideStep:
    """Fused training step of a side model: forward -> soft-target CE -> backward -> RMSprop on one HIP
    stream, every buffer preallocated. A subclass gives the constructor defaults and, in its
    forward_backward, the model's extra forward arguments (`_run`). `class_weight`
    (torch.nn.CrossEntropyLoss(weight=w); train.check_class_weight): the loss launch is f3_soft_ce_w on the
    [N,C] label, torch's rule for probability targets (the weighted sum divided by N); None: f3_soft_ce."""

    def __init__(self, model, batch, lr, alpha, eps, class_weight=None):
        self.model, self.N = model, batch
        self.lr, self.alpha, self.eps = lr, alpha, eps
        dev = model.flat_parameters().device
        nat = model._native
        self.grads = torch.zeros(nat.nparam, dtype=torch.float32, device=dev)
        self.square_avg = torch.zeros(nat.nparam, dtype=torch.float32, device=dev)
        self.ws = torch.empty(nat.workspace_bytes(batch), dtype=torch.uint8, device=dev)
        self.out = torch.empty(batch, model.n_class, dtype=torch.float32, device=dev)
        self.dout = torch.empty_like(self.out)
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)
        self.class_weight = None
        if class_weight is not None:
            from .train import check_class_weight
            self.class_weight = torch.from_numpy(check_class_weight(class_weight, model.n_class)).to(dev)
        grad_views(model, self.grads, self._grad_is_none)

    def _grad_is_none(self, name):
        return False

    def _check(self, x, label):
        who, C = type(self).__name__, self.model.n_class
        self.model.check_inputs(x)
        if x.shape[0] != self.N or not x.is_contiguous() or x.dtype != torch.float32:
            raise ValueError(f"{who}: input must be contiguous fp32 with batch {self.N}")
        if tuple(label.shape) != (self.N, C) or label.dtype != torch.float32 or not label.is_contiguous() \
                or label.device != x.device:
            raise ValueError(f"{who}: label must be contiguous fp32 [{self.N},{C}] on the device")

    def _run(self, x, label, *forward_args):
        """Training forward (with the model's extra arguments), loss and backward on the current stream."""
        m, st = self.model, stream_handle()
        m.native_forward(x, self.out, self.ws, *forward_args, stream=st)
        if self.class_weight is not None:
            check(lib().f3_soft_ce_w(ptr(self.out), ptr(label), None, ptr(self.class_weight), self.N, m.n_class, 0.0,
                                     ptr(self.loss), ptr(self.dout), st), "weighted soft ce")
        else:
            check(lib().f3_soft_ce(ptr(self.out), ptr(label), self.N, m.n_class, ptr(self.loss), ptr(self.dout), st),
                  "soft ce")
        m.native_backward(self.N, self.dout, self.grads, self.ws, st)

    def __call__(self, x, label, *draws, **kwdraws):
        self.forward_backward(x, label, *draws, **kwdraws)
        check(lib().f3_rmsprop_step(ptr(self.model.flat_parameters()), ptr(self.square_avg), ptr(self.grads),
                                    self.grads.numel(), self.lr, self.alpha, self.eps, 1.0, stream_handle()),
              "rmsprop")
        return self.loss
