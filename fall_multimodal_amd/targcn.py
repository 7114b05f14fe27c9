"""TARGCN (BASELINE config 2) as a drop-in module backed by the gfx950 HIP library.

Reference interface mirrored here (file:line relative to /root/reference):
  TARGCN(input_dim=3, num_classes=11, num_nodes=14, ..., adj=None)     TRAGCN.py:177-205
  TARGCN.forward(source[B, T, N, 3]) -> logits[B, num_classes]          TRAGCN.py:207-224
  notebook loop: out = model(pts.permute(0,2,3,1)); CrossEntropyLoss(out, lbs); RMSprop
                                                                        TARGCN_HAR_conv_10kfold.ipynb cell 3

The state_dict has the reference's exact keys, order and shapes (table from f3_targcn_entry):
parameters are views into one flat fp32 buffer (16-B aligned entries), the positional-encoding
table is a buffer. Forward and backward are one native call each (one autograd node); TargcnStep
is the fused forward -> CE -> backward -> RMSprop step with preallocated buffers.

The reference's default adj (Graph(...).A) raises inside its own __init__ and only adj=None works
(SURVEY §0.7); its weights_pool / bias_pool are uninitialised memory (EmbGCN.py:67-68), which is
why its logged run diverges to nan. Here they are initialised U(+-1/sqrt(fan_in)).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from ._flat import FlatModule, NativeHandle, _SideStep
from ._lib import check, lib, ptr, require_device, stream_handle

PRECISION_IDS = {"fp32": 0, "bf16": 1}


def positional_encoding(T=30, F=64):
    """TA.py:75-86."""
    pe = torch.zeros(T, F)
    position = torch.arange(0, T).unsqueeze(1)
    div = torch.exp(torch.arange(0, F, 2) * -(math.log(10000.0) / F))
    pe[:, 0::2] = torch.sin(position * div)
    pe[:, 1::2] = torch.cos(position * div)
    return pe.view(1, T, 1, F)


class _NativeTargcn(NativeHandle):
    def __init__(self, V, num_class, precision):
        if precision not in PRECISION_IDS:
            raise ValueError(f"precision must be one of {sorted(PRECISION_IDS)}, got {precision!r}")
        c = _lib.F3TargcnConfig()
        c.num_node, c.num_class, c.precision = V, num_class, PRECISION_IDS[precision]
        super().__init__("targcn", c)


class TARGCN(FlatModule):
    """TRAGCN.py:177-224 on the MI355X path (adj=None, the only form the reference runs)."""

    def __init__(self, input_dim=3, num_classes=11, num_nodes=14, rnn_units=64, output_dim=64, horizon=30,
                 num_layers=2, embed_dim=64, cheb_k=2, adj=None, device=None, precision="fp32"):
        super().__init__()
        if (input_dim, rnn_units, output_dim, horizon, num_layers, embed_dim) != (3, 64, 64, 30, 2, 64):
            raise NotImplementedError("fall3 TARGCN implements the reference configuration "
                                      "(input_dim 3, rnn_units 64, output_dim 64, horizon 30, 2 layers, embed_dim 64)")
        if adj is not None:
            raise ValueError("TARGCN: only adj=None is supported (the reference's default adj raises, TRAGCN.py:191)")
        object.__setattr__(self, "num_node", num_nodes)
        object.__setattr__(self, "num_class", num_classes)
        object.__setattr__(self, "precision", precision)
        self._build(_NativeTargcn(num_nodes, num_classes, precision), num_classes, device)

    @staticmethod
    def _default(name, shape, shapes):
        """PyTorch default inits of the reference modules; the uninitialised pools get U(+-1/sqrt(fan_in))."""
        leaf = name.rsplit(".", 1)[-1]
        if name.endswith("PE.pe"):
            return positional_encoding()
        if name == "node_embeddings":
            return torch.randn(shape)  # TRAGCN.py:194
        if ".ln" in name:  # LayerNorm: ones / zeros
            return torch.ones(shape) if leaf == "weight" else torch.zeros(shape)
        if leaf == "bias":  # Linear / Conv bias: U(+-1/sqrt(fan_in of its weight))
            fan_in = int(np.prod(shapes[name[: -len("bias")] + "weight"][1:]))
        else:
            fan_in = int(np.prod(shape[1:]))
        b = 1.0 / math.sqrt(fan_in)
        return torch.empty(shape).uniform_(-b, b)

    def check_inputs(self, source):
        require_device(source, "source")
        if source.dim() != 4 or tuple(source.shape[1:]) != (30, self.num_node, 3):
            raise ValueError(f"source must be [B,30,{self.num_node},3], got {tuple(source.shape)}")

    def native_forward(self, source, out, workspace, stream=None):
        st = stream if stream is not None else stream_handle()
        check(lib().f3_targcn_forward(self._native.h, source.shape[0], ptr(self._flat_params),
                                      ptr(self._flat_buffers), ptr(source), ptr(out), ptr(workspace), st),
              "targcn forward")

    def native_backward(self, B, dout, grads, workspace, stream=None):
        st = stream if stream is not None else stream_handle()
        check(lib().f3_targcn_backward(self._native.h, B, ptr(self._flat_params), ptr(self._flat_buffers),
                                       ptr(dout), ptr(grads), ptr(workspace), st), "targcn backward")

    def device_status(self, wait=True):
        """Raise if a GRU group barrier of the last forward / backward timed out (F3_EDEVICE: the
        node-partitioned recurrences' outputs are then wrong); wait=False checks only a completed copy."""
        check(lib().f3_targcn_status(self._native.h, 1 if wait else 0), "targcn device status")

    def forward(self, source):
        """One fall3::targcn_forward custom op (its autograd calls fall3::targcn_backward)."""
        source = source.detach().contiguous().float()
        self.check_inputs(source)
        out, _ = torch.ops.fall3.targcn_forward(self._op_id, list(self.parameters()), self._flat_buffers, source)
        return out


class TargcnStep(_SideStep):
    """Fused TARGCN training step: forward -> soft-target CE -> backward -> RMSprop on one HIP
    stream, every buffer preallocated (the notebook's loop body, TARGCN_HAR_conv_10kfold.ipynb
    cell 3, with its RMSprop(lr=1e-5))."""

    def __init__(self, model: TARGCN, batch, lr=1e-5, alpha=0.99, eps=1e-8, class_weight=None):
        super().__init__(model, batch, lr, alpha, eps, class_weight)

    def forward_backward(self, source, label):
        self._check(source, label)
        self._run(source, label)

    def __call__(self, source, label):
        # a flagged barrier of an earlier step surfaces here (or from the native calls themselves)
        self.model.device_status(wait=False)
        return super().__call__(source, label)
