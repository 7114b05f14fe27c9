"""musa_model.Model (the model the root Multimodal_Fall3/main.py trains) as a drop-in module backed
by the gfx950 HIP library.

Reference interface mirrored here (file:line relative to /root/reference/Multimodal_Fall3):
  adjGraph(layout='coco_cut', strategy='uniform')                 model/musa_model.py:200-349
  Model(num_class, num_point, max_frame, graph, bias, edge, block_size, embed_dim=64, n_stage=1,
        act_type='tanh')                                          model/musa_model.py:492-559
  Model.forward(x[N, 3, T, V]) -> logits[N, num_class]            model/musa_model.py:561-589
  driver: Model(num_class=11, num_point=14, max_frame=300, graph=adjGraph('coco_cut','uniform'),
          bias=True, edge=True, block_size=41, embed_dim=64, n_stage=1, act_type='tanh')
                                                                  main.py:307-320

The state_dict has the reference's exact keys, order and shapes (f3_musa_entry), A included (a
Parameter with requires_grad=False, as the reference registers it). Train-mode randomness: the
DropBlocks (keep_prob 0.9 at musa_model.py:509) and the head's Dropout(0.2) are drawn in the kernels
from a counter hash of a per-step seed taken from the module's generator (the oracle reproduces the
draws); `dropblock=False` runs the reference with keep_prob 1 and p 0.
"""
from __future__ import annotations

import ctypes
import re
import math

import numpy as np
import torch

from . import _lib
from ._flat import FlatModule, NativeHandle, _SideStep
from ._lib import check, lib, ptr, require_device, stream_handle


class adjGraph:  # noqa: N801  (reference name)
    """musa_model.py:200-349 for the layouts / strategies the driver uses: 'coco_cut' with 'uniform'
    (normalize_digraph of the 1-hop adjacency incl. self links), A of shape [1, V, V]."""

    def __init__(self, layout="coco_cut", strategy="uniform", max_hop=1, dilation=1):
        if layout != "coco_cut" or strategy != "uniform" or max_hop != 1 or dilation != 1:
            raise NotImplementedError("fall3 adjGraph: layout 'coco_cut', strategy 'uniform' (the driver's graph)")
        V = 14
        edges = [(i, i) for i in range(V)] + [(6, 4), (4, 2), (2, 13), (13, 1), (5, 3), (3, 1), (12, 10), (10, 8),
                                              (8, 2), (11, 9), (9, 7), (7, 1), (13, 0)]
        A = np.zeros((V, V))
        for i, j in edges:
            A[j, i] = A[i, j] = 1
        Dl = A.sum(0)
        Dn = np.diag([d ** -1 if d > 0 else 0 for d in Dl])
        self.num_node = V
        self.A = (A @ Dn)[None]


class _NativeMusa(NativeHandle):
    def __init__(self, V, T, num_class, precision=0):
        c = _lib.F3MusaConfig()
        c.num_point, c.frames, c.num_class, c.precision = V, T, num_class, precision
        super().__init__("musa", c)


class Model(FlatModule):
    """musa_model.Model on the MI355X path (the driver's configuration)."""

    def __init__(self, num_class, num_point, max_frame, graph, bias, edge, block_size, embed_dim=64, n_stage=1,
                 act_type="tanh", device=None, dropblock=True, seed=0, frames=30, precision="fp32"):
        """precision: "fp32" (fp32 MFMA; the parity mode) or "bf16" (the root main.py trains under bf16
        autocast, Multimodal_Fall3/main.py:97: the streams' 1x1 convs on bf16 MFMA with fp32 accumulate;
        depthwise convs, graph mix, BatchNorms, DropBlock and the head stay fp32)."""
        super().__init__()
        if precision not in ("fp32", "bf16"):
            raise ValueError(f"precision must be 'fp32' or 'bf16', got {precision!r}")
        object.__setattr__(self, "precision", precision)
        if (embed_dim, n_stage, act_type, bool(bias), bool(edge), block_size) != (64, 1, "tanh", True, True, 41):
            raise NotImplementedError("fall3 musa Model implements the driver's configuration (embed_dim 64, "
                                      "n_stage 1, act 'tanh', bias, edge, block_size 41; main.py:307-320)")
        A = np.asarray(graph.A, dtype=np.float32)
        if A.shape != (1, num_point, num_point):
            raise ValueError(f"graph.A must be [1, {num_point}, {num_point}] (uniform strategy), got {A.shape}")
        object.__setattr__(self, "num_classes", num_class)
        object.__setattr__(self, "num_point", num_point)
        object.__setattr__(self, "frames", frames)
        object.__setattr__(self, "dropblock", bool(dropblock))
        object.__setattr__(self, "_gen", torch.Generator().manual_seed(int(seed)))
        object.__setattr__(self, "_graph_A", A)
        self._build(_NativeMusa(num_point, frames, num_class, 1 if precision == "bf16" else 0), num_class, device)

    def _requires_grad(self, name):
        return not name.endswith(".A")  # the reference registers A as a frozen Parameter

    def _default(self, name, shape, shapes):
        """The graph for A, else PyTorch default inits (init_param at musa_model.py:408-420 is never called)."""
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "A":
            return torch.from_numpy(self._graph_A)
        if leaf == "edge":
            return torch.ones(shape)
        if leaf == "running_mean":
            return torch.zeros(shape)
        if leaf == "running_var":
            return torch.ones(shape)
        if leaf == "num_batches_tracked":
            return torch.zeros(shape, dtype=torch.int64)
        if len(shape) == 1 and leaf == "weight":   # BatchNorm / LayerNorm affine
            return torch.ones(shape)
        if len(shape) == 1 and leaf == "bias" and (name[: -len("bias")] + "weight") in shapes \
                and len(shapes[name[: -len("bias")] + "weight"]) == 1:
            return torch.zeros(shape)
        if leaf == "bias":
            fan_in = int(np.prod(shapes[name[: -len("bias")] + "weight"][1:]))
        else:
            fan_in = int(np.prod(shape[1:]))
        b = 1.0 / math.sqrt(fan_in)
        return torch.empty(shape).uniform_(-b, b)

    def check_inputs(self, x):
        require_device(x, "x")
        want = (3, self.frames, self.num_point)
        if x.dim() != 4 or tuple(x.shape[1:]) != want:
            raise ValueError(f"x must be [N,{','.join(map(str, want))}], got {tuple(x.shape)}")

    def draw_seed(self):
        return int(torch.randint(0, 2 ** 31 - 1, (), generator=self._gen).item())

    def native_forward(self, x, out, workspace, training, seed=0, buffers=None, counters=None, stream=None):
        st = stream if stream is not None else stream_handle()
        b = self._flat_buffers if buffers is None else buffers
        c = self._counters if counters is None else counters
        check(lib().f3_musa_forward(self._native.h, x.shape[0], int(training), ptr(self._flat_params), ptr(b), ptr(c),
                                    ptr(x), ptr(out), ptr(workspace), ctypes.c_uint(seed & 0xFFFFFFFF),
                                    int(training and self.dropblock), st), "musa forward")

    def native_backward(self, B, dout, grads, workspace, stream=None):
        st = stream if stream is not None else stream_handle()
        check(lib().f3_musa_backward(self._native.h, B, ptr(self._flat_params), ptr(self._flat_buffers), ptr(dout),
                                     ptr(grads), ptr(workspace), st), "musa backward")

    def forward(self, x):
        """One fall3::musa_forward custom op (its autograd calls fall3::musa_backward)."""
        x = x.detach().contiguous().float()
        self.check_inputs(x)
        seed = self.draw_seed() if self.training else 0
        out, _, nb, nc = torch.ops.fall3.musa_forward(self._op_id, list(self.parameters()), self._flat_buffers,
                                                      self._counters, x, self.training, seed)
        if self.training:
            with torch.no_grad():
                self._flat_buffers.copy_(nb)
                self._counters.copy_(nc)
        return out


_FROZEN = re.compile(r"(^|\.)A$")
_SEP_EDGE = re.compile(r"^stream_(pos|mot)\.[12]\.edge$")


def grad_is_none(name, dropblock_active):
    """True for the parameters whose .grad the reference leaves None after backward.
    * The graphs `A` (requires_grad False): always.
    * The SepTemporal blocks' `edge` (musa_model.py:184-198): it enters the graph only through
      Randomized_DropBlock_Ske's M = matmul(M_seed, A * edge), whose every element the masked writes
      `M[M > 0.001] = 1.0; M[M < 0.5] = 0.0` (musa_model.py:66-69) then overwrite with a constant.
      With DropBlock active (training, keep_prob < 1: the driver's 0.9, musa_model.py:510) autograd
      therefore gives edge an all-ZERO gradient tensor - so weight-decaying optimizers (the
      reference's SGD / Adam / AdamW builders) still move it and keep state for it. Without DropBlock
      (keep_prob 1, eval) edge is unused and its gradient stays None. f3_musa_backward zero-fills
      these slots either way."""
    if _FROZEN.search(name):
        return True
    return bool(_SEP_EDGE.search(name)) and not dropblock_active


class MusaStep(_SideStep):
    """Fused musa_model training step: forward -> soft-target CE -> backward -> RMSprop on one HIP
    stream with preallocated buffers (main.py's train loop body with RMSprop(lr=1e-3))."""

    def __init__(self, model: Model, batch, lr=1e-3, alpha=0.99, eps=1e-8, class_weight=None):
        super().__init__(model, batch, lr, alpha, eps, class_weight)
        self.last_seed = None

    def _grad_is_none(self, name):
        # A (frozen) has no gradient; the SepTemporal blocks' edges get the zero gradient the
        # reference's DropBlock gives them (None without DropBlock). RMSprop maps a zero gradient
        # to a zero update (square_avg stays 0), as torch.optim.RMSprop (no weight decay) does
        return grad_is_none(name, self.model.dropblock)

    def forward_backward(self, x, label, seed=None):
        self._check(x, label)
        seed = self.model.draw_seed() if seed is None else int(seed)
        self.last_seed = seed
        self._run(x, label, True, seed)
