"""PyTorch custom ops (torch.library) over the C ABI: the boundary SURVEY §8(b) names
(`TORCH_LIBRARY(fall3, m)`-style ops with fake kernels and autograd), so the native step works
under torch.compile / FakeTensor tracing and composes with the rest of an autograd graph.

  fall3::net_forward(net, params, buffers, counters, skel?, sensor?, training)
        -> (out, workspace, new running buffers, new counters)
        model(data, sensor), Multimodal_Fall3/model/main.py:112 (combination.py:37-46)
  fall3::net_backward(net, params, dout, workspace) -> grads (flat, params layout)
        loss.backward(), main.py:115
  fall3::targcn_forward(net, params, buffers, source) -> (out, workspace)
        model(pts.permute(0,2,3,1)), TARGCN_HAR_conv_10kfold.ipynb cell 3 (TRAGCN.py:207-224)
  fall3::targcn_backward(net, params, buffers, dout, workspace) -> grads
  fall3::sktr_forward(net, params, buffers, counters, x, training, sd, seed)
        -> (out, workspace, new running buffers, new counters)
        model(x), skeleton_transformer.py:418-435 (BASELINE config 5)
  fall3::sktr_backward(net, params, dout, workspace) -> grads
  fall3::musa_forward(net, params, buffers, counters, x, training, seed) -> (out, workspace, buffers, counters)
        model(data), Multimodal_Fall3/model/musa_model.py:561-589 (root main.py:97-99)
  fall3::musa_backward(net, params, dout, workspace) -> grads
  fall3::rmsprop_(param!, square_avg!, grad, lr, alpha, eps, scale)
        optimizer.step(), model/optimizer.py:21 (torch.optim.RMSprop semantics)
  fall3::optim_(param!, state0!, state1!, scalars!, grad, kind, nesterov, lr, alpha, eps, momentum, beta1, beta2,
                weight_decay, max_norm, grad_scale, skip)
        [clip_grad_norm_;] optimizer.step() for torch.optim.SGD / Adam / AdamW / RMSprop with weight decay,
        model/optimizer.py:20-29, root main.py:108-113 (f3_optim_step)

`net` is the integer id of a live native model (its f3_net / f3_targcn handle); `params` is the
module's parameter list (views of one flat buffer, which the native call reads through). The ops
are functional (an op that mutates its inputs cannot carry an autograd formula): net_forward
returns the updated BatchNorm running statistics / counters, which the module copies back as
nn.BatchNorm updates them in place. Fake kernels return outputs of the right shapes without
touching the device; the workspace size comes from the host-side plan (f3_*_workspace_bytes).
"""
from __future__ import annotations

import weakref
from typing import List, Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from ._lib import check, lib, ptr, stream_handle

_NETS: "weakref.WeakValueDictionary[int, object]" = weakref.WeakValueDictionary()


def register(module) -> int:
    """Make a native-backed module reachable from the ops; returns its id."""
    key = id(module)
    _NETS[key] = module
    return key


def _module(net: int):
    m = _NETS.get(net)
    if m is None:
        raise RuntimeError(f"fall3 op: no live native model with id {net}")
    return m


# ---------------------------------------------------------------------------------------------
# bodies the four models' ops share
# ---------------------------------------------------------------------------------------------
def _out_ws(m, ref):
    """(logits, workspace) for the batch of `ref`, on its device."""
    N = ref.shape[0]
    return (torch.empty(N, m.n_class, dtype=torch.float32, device=ref.device),
            torch.empty(m._native.workspace_bytes(N), dtype=torch.uint8, device=ref.device))


def _fake_out_ws(m, ref):
    N = ref.shape[0]
    return (ref.new_empty(N, m.n_class, dtype=torch.float32),
            ref.new_empty(m._native.workspace_bytes(N), dtype=torch.uint8))


def _clone_state(buffers, counters):
    """The copies a functional forward updates in place of the module's running statistics / counters."""
    return buffers.clone(), counters.clone()


def _flat_backward(net, dout, workspace):
    """The model's native backward into a fresh flat gradient (params layout)."""
    m = _module(net)
    grads = torch.empty(m._native.nparam, dtype=torch.float32, device=dout.device)
    m.native_backward(dout.shape[0], dout.contiguous(), grads, workspace)
    return grads


def _fake_flat_backward(net, dout):
    return dout.new_empty(_module(net)._native.nparam, dtype=torch.float32)


def _no_grad_outputs(ctx, output):
    """The workspace and the new running buffers / counters carry no gradient. Without this autograd
    materialises a zero gradient for each of them before calling backward: for the ~9 GB workspace
    that is a 1 ms fill per step (4 x 245 us `FillFunctor<unsigned char>` launches in the rocprof
    trace of the unchanged main.py loop)."""
    ctx.set_materialize_grads(False)
    ctx.mark_non_differentiable(*output[1:])


def _split_grads(m, grads):
    """Views of the flat gradient in parameter order (the (shape, stride, offset) table is built once
    per module; as_strided is the cheapest per-view call, ~1.3 us against ~3 us for slice + view)."""
    table = getattr(m, "_f3_grad_table", None)
    if table is None:
        table = []
        for _, shape, off in m.param_views():
            shape = tuple(int(d) for d in shape)
            stride, acc = [], 1
            for d in reversed(shape):
                stride.append(acc)
                acc *= d
            table.append((shape, tuple(reversed(stride)), int(off)))
        object.__setattr__(m, "_f3_grad_table", table)
    o0 = grads.storage_offset()
    return [grads.as_strided(shape, stride, o0 + off) for shape, stride, off in table]


def _training_backward(ctx, dout, backward_op):
    """Parameter gradients of a forward that saved its workspace (training mode only)."""
    if not ctx.training:
        raise RuntimeError("fall3: backward through an eval-mode forward is not supported")
    (ws,) = ctx.saved_tensors
    m = _module(ctx.net)
    return m, _split_grads(m, backward_op(ctx.net, list(m.parameters()), dout.float(), ws))


# ---------------------------------------------------------------------------------------------
# 3-stream / 2-stream / single-stream / sensor models (f3_net)
# ---------------------------------------------------------------------------------------------
@torch.library.custom_op("fall3::net_forward", mutates_args=())
def net_forward(net: int, params: List[Tensor], buffers: Tensor, counters: Tensor, skel: Optional[Tensor],
                sensor: Optional[Tensor], training: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Functional: returns (out, workspace, new running buffers, new counters); the module copies the
    new BatchNorm running statistics back (a mutating op could not carry an autograd formula)."""
    m = _module(net)
    out, ws = _out_ws(m, skel if skel is not None else sensor)
    nb, nc = _clone_state(buffers, counters)
    m.native_forward(skel, sensor, out, ws, training, buffers=nb, counters=nc)
    return out, ws, nb, nc


@net_forward.register_fake
def _(net, params, buffers, counters, skel, sensor, training):
    return (*_fake_out_ws(_module(net), skel if skel is not None else sensor), torch.empty_like(buffers),
            torch.empty_like(counters))


@torch.library.custom_op("fall3::net_backward", mutates_args=())
def net_backward(net: int, params: List[Tensor], dout: Tensor, workspace: Tensor) -> Tensor:
    return _flat_backward(net, dout, workspace)


@net_backward.register_fake
def _(net, params, dout, workspace):
    return _fake_flat_backward(net, dout)


def _net_setup(ctx, inputs, output):
    ctx.net, ctx.training = inputs[0], inputs[6]
    ctx.save_for_backward(output[1])
    _no_grad_outputs(ctx, output)


def _net_backward(ctx, dout, dws, dbuf, dcnt):
    _, gl = _training_backward(ctx, dout, torch.ops.fall3.net_backward)
    return None, gl, None, None, None, None, None


net_forward.register_autograd(_net_backward, setup_context=_net_setup)


# ---------------------------------------------------------------------------------------------
# TARGCN (f3_targcn)
# ---------------------------------------------------------------------------------------------
@torch.library.custom_op("fall3::targcn_forward", mutates_args=())
def targcn_forward(net: int, params: List[Tensor], buffers: Tensor, source: Tensor) -> Tuple[Tensor, Tensor]:
    m = _module(net)
    out, ws = _out_ws(m, source)
    m.native_forward(source, out, ws)
    return out, ws


@targcn_forward.register_fake
def _(net, params, buffers, source):
    return _fake_out_ws(_module(net), source)


@torch.library.custom_op("fall3::targcn_backward", mutates_args=())
def targcn_backward(net: int, params: List[Tensor], buffers: Tensor, dout: Tensor, workspace: Tensor) -> Tensor:
    return _flat_backward(net, dout, workspace)


@targcn_backward.register_fake
def _(net, params, buffers, dout, workspace):
    return _fake_flat_backward(net, dout)


def _tg_setup(ctx, inputs, output):
    ctx.net = inputs[0]
    ctx.save_for_backward(inputs[2], output[1])
    _no_grad_outputs(ctx, output)


def _tg_backward(ctx, dout, dws):
    buffers, ws = ctx.saved_tensors
    m = _module(ctx.net)
    grads = torch.ops.fall3.targcn_backward(ctx.net, list(m.parameters()), buffers, dout.float(), ws)
    return None, _split_grads(m, grads), None, None


targcn_forward.register_autograd(_tg_backward, setup_context=_tg_setup)


# ---------------------------------------------------------------------------------------------
# SkeletonTransformer (f3_sktr)
# ---------------------------------------------------------------------------------------------
@torch.library.custom_op("fall3::sktr_forward", mutates_args=())
def sktr_forward(net: int, params: List[Tensor], buffers: Tensor, counters: Tensor, x: Tensor, training: bool,
                 sd: List[float], seed: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Functional like net_forward: returns the new BatchNorm3d running statistics / counters."""
    m = _module(net)
    out, ws = _out_ws(m, x)
    nb, nc = _clone_state(buffers, counters)
    m.native_forward(x, out, ws, training, sd, seed, buffers=nb, counters=nc)
    return out, ws, nb, nc


@sktr_forward.register_fake
def _(net, params, buffers, counters, x, training, sd, seed):
    return (*_fake_out_ws(_module(net), x), torch.empty_like(buffers), torch.empty_like(counters))


@torch.library.custom_op("fall3::sktr_backward", mutates_args=())
def sktr_backward(net: int, params: List[Tensor], dout: Tensor, workspace: Tensor) -> Tensor:
    return _flat_backward(net, dout, workspace)


@sktr_backward.register_fake
def _(net, params, dout, workspace):
    return _fake_flat_backward(net, dout)


def _sk_setup(ctx, inputs, output):
    ctx.net, ctx.training = inputs[0], inputs[5]
    ctx.save_for_backward(output[1])
    _no_grad_outputs(ctx, output)


def _sk_backward(ctx, dout, dws, dbuf, dcnt):
    _, gl = _training_backward(ctx, dout, torch.ops.fall3.sktr_backward)
    return None, gl, None, None, None, None, None, None


sktr_forward.register_autograd(_sk_backward, setup_context=_sk_setup)


# ---------------------------------------------------------------------------------------------
# musa_model.Model (f3_musa)
# ---------------------------------------------------------------------------------------------
@torch.library.custom_op("fall3::musa_forward", mutates_args=())
def musa_forward(net: int, params: List[Tensor], buffers: Tensor, counters: Tensor, x: Tensor, training: bool,
                 seed: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    m = _module(net)
    out, ws = _out_ws(m, x)
    nb, nc = _clone_state(buffers, counters)
    m.native_forward(x, out, ws, training, seed, buffers=nb, counters=nc)
    return out, ws, nb, nc


@musa_forward.register_fake
def _(net, params, buffers, counters, x, training, seed):
    return (*_fake_out_ws(_module(net), x), torch.empty_like(buffers), torch.empty_like(counters))


@torch.library.custom_op("fall3::musa_backward", mutates_args=())
def musa_backward(net: int, params: List[Tensor], dout: Tensor, workspace: Tensor) -> Tensor:
    return _flat_backward(net, dout, workspace)


@musa_backward.register_fake
def _(net, params, dout, workspace):
    return _fake_flat_backward(net, dout)


def _mu_backward(ctx, dout, dws, dbuf, dcnt):
    m, gl = _training_backward(ctx, dout, torch.ops.fall3.musa_backward)
    from .musa import grad_is_none
    # None where the reference's autograd leaves None: A (frozen) always, the SepTemporal edges
    # unless DropBlock ran (then the reference gives them a zero tensor; musa.grad_is_none)
    gl = [None if grad_is_none(name, m.dropblock) else g for g, (name, _, _) in zip(gl, m.param_views())]
    return None, gl, None, None, None, None, None


musa_forward.register_autograd(_mu_backward, setup_context=_sk_setup)


# ---------------------------------------------------------------------------------------------
# RMSprop update (in place)
# ---------------------------------------------------------------------------------------------
@torch.library.custom_op("fall3::rmsprop_", mutates_args=("param", "square_avg"))
def rmsprop_(param: Tensor, square_avg: Tensor, grad: Tensor, lr: float, alpha: float, eps: float,
             scale: float) -> None:
    if not (param.is_contiguous() and square_avg.is_contiguous() and grad.is_contiguous()):
        raise RuntimeError("fall3 rmsprop_: contiguous tensors required")
    check(lib().f3_rmsprop_step(ptr(param), ptr(square_avg), ptr(grad), param.numel(), lr, alpha, eps, scale,
                                stream_handle()), "rmsprop")


@rmsprop_.register_fake
def _(param, square_avg, grad, lr, alpha, eps, scale):
    return None


# ---------------------------------------------------------------------------------------------
# SGD / Adam / AdamW / RMSprop with weight decay, optional grad-norm clipping (in place)
# ---------------------------------------------------------------------------------------------
def optim_config(kind: int, nesterov: bool, lr: float, alpha: float, eps: float, momentum: float, beta1: float,
                 beta2: float, weight_decay: float, max_norm: float, grad_scale: float, skip=(), skip_nonfinite=False):
    """f3_optim_config from Python values; skip = flat [lo0, len0, lo1, len1, ...] of the no-gradient ranges;
    skip_nonfinite: the update is skipped on the device when the gradient holds an inf or NaN (guard_views)."""
    c = _lib.F3OptimConfig()
    c.kind, c.nesterov = int(kind), int(bool(nesterov))
    c.skip_nonfinite = int(bool(skip_nonfinite))
    c.lr, c.alpha, c.eps, c.momentum = lr, alpha, eps, momentum
    c.beta1, c.beta2, c.weight_decay, c.max_norm, c.grad_scale = beta1, beta2, weight_decay, max_norm, grad_scale
    if len(skip) % 2 or len(skip) // 2 > _lib.OPT_MAX_SKIP:
        raise RuntimeError(f"fall3 optim_: at most {_lib.OPT_MAX_SKIP} (lo, len) skip ranges")
    c.nskip = len(skip) // 2
    for j in range(c.nskip):
        c.skip_lo[j], c.skip_len[j] = int(skip[2 * j]), int(skip[2 * j + 1])
    return c


def optim_scalars(device):
    """A zeroed step-scalar block (f3_optim_scalars_bytes) as an fp32 tensor; see scalar_views."""
    return torch.zeros(int(lib().f3_optim_scalars_bytes()) // 4, dtype=torch.float32, device=device)


def scalar_views(scalars: Tensor):
    """(t int64[1], bias_correction1, bias_correction2_sqrt, clip_coef, grad_norm: fp32[1] each) views of a
    step-scalar block, in the layout include/fall3.h documents."""
    return (scalars[0:2].view(torch.int64), scalars[2:3], scalars[3:4], scalars[4:5], scalars[5:6])


def guard_views(scalars: Tensor):
    """(skipped int64[1], last_skipped int32[1]) views of a step-scalar block: the number of updates a
    guarded step (skip_nonfinite) has skipped since the block was zeroed, and whether the last one was."""
    o = int(lib().f3_optim_guard_offset()) // 4
    return scalars[o:o + 2].view(torch.int64), scalars[o + 2:o + 3].view(torch.int32)


HYPER_FIELDS = ("lr", "alpha", "eps", "momentum", "beta1", "beta2", "weight_decay", "max_norm", "grad_scale")


def optim_hyper(device):
    """A zeroed hyper-parameter block (f3_optim_hyper_bytes) as an fp64 tensor; f3_optim_hyper_set writes
    it, the update launches of f3_optim_step_hyper read it."""
    return torch.zeros(int(lib().f3_optim_hyper_bytes()) // 8, dtype=torch.float64, device=device)


def hyper_views(block: Tensor):
    """The block's values as a float64 view, in HYPER_FIELDS order (the layout include/fall3.h documents)."""
    return block.view(torch.float64)[:len(HYPER_FIELDS)]


def ema_state(device):
    """A zeroed EMA block (f3_ema_state_bytes) as an int64 tensor; f3_ema_set_decay writes its decay, every
    f3_ema_update reads it and advances its count; see ema_views."""
    return torch.zeros(int(lib().f3_ema_state_bytes()) // 8, dtype=torch.int64, device=device)


def ema_views(block: Tensor):
    """(n_averaged int64[1], decay fp64[1]) views of an EMA block, in the layout include/fall3.h documents."""
    return block[0:1], block[1:2].view(torch.float64)


@torch.library.custom_op("fall3::optim_", mutates_args=("param", "state0", "state1", "scalars"))
def optim_(param: Tensor, state0: Tensor, state1: Tensor, scalars: Tensor, grad: Tensor, kind: int, nesterov: bool,
           lr: float, alpha: float, eps: float, momentum: float, beta1: float, beta2: float, weight_decay: float,
           max_norm: float, grad_scale: float, skip: List[int]) -> None:
    """state0 / state1 with no elements stand for "no such state" (SGD without momentum; state1 of
    every kind but Adam / AdamW)."""
    for t in (param, state0, state1, grad):
        if not t.is_contiguous():
            raise RuntimeError("fall3 optim_: contiguous tensors required")
    c = optim_config(kind, nesterov, lr, alpha, eps, momentum, beta1, beta2, weight_decay, max_norm, grad_scale, skip)
    s0 = state0 if state0.numel() else None
    s1 = state1 if state1.numel() else None
    check(lib().f3_optim_step(c, ptr(param), ptr(s0), ptr(s1), ptr(grad), param.numel(), ptr(scalars),
                              stream_handle()), "optim step")


@optim_.register_fake
def _(param, state0, state1, scalars, grad, kind, nesterov, lr, alpha, eps, momentum, beta1, beta2, weight_decay,
      max_norm, grad_scale, skip):
    return None
