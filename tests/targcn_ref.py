"""High-precision references and the per-tensor gradient gate for the TARGCN step (plain helpers, no fixtures).

  oracle_fp64           oracle.targcn_cpu.train_step with state, source and label in float64
  oracle_bf16_operands  the same fp64 step with the GEMM operands rounded to bf16 (straight-through for
                        autograd): the reference's own response to bf16 operand rounding, nothing of the
                        code under test in it
  envelope              per tensor, max|gbf - g64| / max|g64|
  gate                  per tensor, max|ours - g64| / max|g64| <= tol

Tolerances (chosen from the reference and the project, before any kernel was measured against them):
fp32 mode: every gradient within FP32_GRAD_TOL = 1e-4 of its tensor's max (the project's fp32-vs-fp32
summation-order bar, tests/test_gpu_cnn1d.py), logits and loss within 1e-5. bf16 mode: tol_k =
MARGIN * max(env_k, median(env)) with MARGIN = 4; a tensor whose tol_k exceeds CAP = 0.25 is left out of the
per-tensor gate for that case (covered by the cosine), at most MAX_LEFT_OUT of them.

Results are cached per (V, B, num_class, seeds): the modes of one case share one oracle run.
"""
import os
from collections import OrderedDict

import numpy as np
import torch

from oracle import targcn_cpu as tg

SEED_STATE, SEED_DATA = 11, 5
FP32_GRAD_TOL = 1e-4
FP32_LOGIT_TOL = 1e-5
FP32_LOSS_TOL = 1e-5
MARGIN = 4.0
CAP = 0.25
MAX_LEFT_OUT = 4

# (V, B, num_class): the edge shapes of tests/test_gpu_targcn_edges.py, with the number of tensors the
# reference's own bf16 response puts over the cap (an upper bound, asserted by tests/test_targcn_ref.py)
CASES = [(2, 1, 11), (16, 5, 11), (18, 33, 11), (17, 65, 11), (14, 3, 64), (14, 3, 2)]
OVER_CAP = {(2, 1, 11): 2, (16, 5, 11): 0, (18, 33, 11): 0, (17, 65, 11): 0, (14, 3, 64): 0, (14, 3, 2): 0}

_CACHE = {}


def _threads():
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def inputs(V, B, num_class, seed_state=SEED_STATE, seed_data=SEED_DATA):
    """(state, source, label) of one case: fp32 tensors / arrays, as the device step gets them."""
    st = tg.init_state(V, seed_state, num_class)
    src, label = tg.synthetic_source(B, V, num_class, seed_data)
    return st, src, label


def _step(V, B, num_class, seed_state, seed_data, dtype):
    _threads()
    st, src, label = inputs(V, B, num_class, seed_state, seed_data)
    st = OrderedDict((k, v.to(dtype)) for k, v in st.items())
    out, loss, grads = tg.train_step(st, torch.from_numpy(src).to(dtype), torch.from_numpy(label).to(dtype))
    return {"out": out.numpy().astype(np.float64), "loss": float(loss),
            "grads": OrderedDict((k, g.numpy().astype(np.float64)) for k, g in grads.items())}


def oracle_fp64(V, B, num_class, seed_state=SEED_STATE, seed_data=SEED_DATA):
    """The oracle's training step in float64: {"out": logits, "loss": float, "grads": {name: array}}."""
    key = ("fp64", V, B, num_class, seed_state, seed_data)
    if key not in _CACHE:
        _CACHE[key] = _step(V, B, num_class, seed_state, seed_data, torch.float64)
    return _CACHE[key]


def oracle_fp32(V, B, num_class, seed_state=SEED_STATE, seed_data=SEED_DATA):
    """The oracle's training step as it is written (fp32), for the gate's own CPU tests."""
    key = ("fp32", V, B, num_class, seed_state, seed_data)
    if key not in _CACHE:
        _CACHE[key] = _step(V, B, num_class, seed_state, seed_data, torch.float32)
    return _CACHE[key]


def _bf16(x):
    """Round to bf16 in the forward, identity in the backward."""
    return x + (x.bfloat16().to(x.dtype) - x).detach()


class _Rounded(dict):
    """A view of a state dict whose listed entries read as bf16-rounded."""

    def __init__(self, st, keys):
        super().__init__()
        self._st, self._keys = st, keys

    def __getitem__(self, k):
        v = self._st[k]
        return _bf16(v) if k in self._keys else v


def oracle_bf16_operands(V, B, num_class, seed_state=SEED_STATE, seed_data=SEED_DATA):
    """The fp64 step with the GEMM operands rounded to bf16: EmbGCN's x, weights_pool and linear.weight,
    Transform's x and its conv1 / conv2 / vff / ff.0 / ff.2 weights. Same return as oracle_fp64."""
    key = ("bf16op", V, B, num_class, seed_state, seed_data)
    if key in _CACHE:
        return _CACHE[key]
    embgcn, transform = tg.embgcn, tg.transform

    def embgcn_r(st, p, x, E, S, cs):
        return embgcn(_Rounded(st, {p + "weights_pool", p + "linear.weight"}), p, _bf16(x), E, S, cs)

    def transform_r(st, p, x):
        keys = {p + n + ".weight" for n in ("conv1", "conv2", "vff", "ff.0", "ff.2")}
        return transform(_Rounded(st, keys), p, _bf16(x))

    tg.embgcn, tg.transform = embgcn_r, transform_r
    try:
        _CACHE[key] = _step(V, B, num_class, seed_state, seed_data, torch.float64)
    finally:
        tg.embgcn, tg.transform = embgcn, transform
    return _CACHE[key]


def _ratio(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))


def envelope(g64, gbf):
    """Per tensor, env_k = max|gbf_k - g64_k| / max|g64_k|."""
    return OrderedDict((k, _ratio(gbf[k], g64[k])) for k in g64)


def bf16_tolerances(env):
    """(tol, left_out): tol_k = MARGIN * max(env_k, median(env)) for the gated tensors; the tensors whose
    tol_k exceeds CAP are left out (at most MAX_LEFT_OUT)."""
    med = float(np.median(list(env.values())))
    tol = OrderedDict((k, MARGIN * max(e, med)) for k, e in env.items())
    left_out = [k for k, t in tol.items() if t > CAP]
    assert len(left_out) <= MAX_LEFT_OUT, (left_out, [tol[k] for k in left_out])
    return OrderedDict((k, t) for k, t in tol.items() if t <= CAP), left_out


def ratios(ours, g64):
    assert set(ours) == set(g64), set(ours) ^ set(g64)
    return OrderedDict((k, _ratio(ours[k], g64[k])) for k in g64)


def gate(ours, g64, tol, what=""):
    """Assert max|ours_k - g64_k| / max|g64_k| <= tol_k for every tensor of `tol` (a mapping name -> bound,
    or one bound for every tensor), naming every failing tensor with its ratio. Returns all the ratios."""
    r = ratios(ours, g64)
    bound = tol if isinstance(tol, dict) else {k: float(tol) for k in g64}
    bad = [(k, r[k], bound[k]) for k in bound if not r[k] <= bound[k]]  # (a NaN ratio fails)
    assert not bad, what + " gradient gate: " + "; ".join(f"{k} {v:.3e} > {b:.3e}" for k, v, b in bad)
    return r


def cosine(ours, g64):
    a = np.concatenate([np.asarray(ours[k], np.float64).reshape(-1) for k in g64])
    r = np.concatenate([np.asarray(g64[k], np.float64).reshape(-1) for k in g64])
    return float(a @ r / (np.linalg.norm(a) * np.linalg.norm(r)))


def bf16_reference(V, B, num_class, seed_state=SEED_STATE, seed_data=SEED_DATA):
    """What the bf16 gate of one case needs: (fp64 result, env, tol, left_out, emulated max|dlogit|)."""
    r64 = oracle_fp64(V, B, num_class, seed_state, seed_data)
    rbf = oracle_bf16_operands(V, B, num_class, seed_state, seed_data)
    env = envelope(r64["grads"], rbf["grads"])
    tol, left_out = bf16_tolerances(env)
    return r64, env, tol, left_out, float(np.abs(rbf["out"] - r64["out"]).max())
