"""Native SGD / Adam / AdamW / RMSprop-with-decay: everything that needs no GPU.

`ref_step` is the fp64 restatement of the update formulas of include/fall3.h (f3_optim_config). It is
pinned to torch.optim here, on fp64 CPU tensors, and tests/test_gpu_optim.py then holds the HIP
kernels to it. Also: the flat-buffer <-> state_dict conversions on fabricated buffers,
build_optimizer's classes, and the settings that are refused."""
import math
from types import SimpleNamespace

import pytest
import torch

from fall_multimodal_amd import optim as fo


def ref_step(kind, p, state, grad, t, *, lr, alpha=0.99, eps=1e-8, momentum=0.0, nesterov=False,
             betas=(0.9, 0.999), weight_decay=0.0, grad_scale=1.0, clip_coef=1.0):
    """One optimizer step in fp64. p, grad: tensors; state: dict of torch's state tensors (missing =
    zeros); t: the step number of THIS step (1-based; Adam's bias corrections). Returns (p, state)."""
    p = p.double()
    g = grad_scale * clip_coef * grad.double()
    z = torch.zeros_like(p)
    new = {}
    if kind == "adamw":
        p = p * (1 - lr * weight_decay)
    else:
        g = g + weight_decay * p
    if kind == "rmsprop":
        sq = alpha * state.get("square_avg", z).double() + (1 - alpha) * g * g
        new["square_avg"] = sq
        p = p - lr * g / (sq.sqrt() + eps)
    elif kind == "sgd":
        if momentum != 0:
            buf = momentum * state.get("momentum_buffer", z).double() + g
            new["momentum_buffer"] = buf
            d = g + momentum * buf if nesterov else buf
        else:
            d = g
        p = p - lr * d
    else:
        b1, b2 = betas
        m0 = state.get("exp_avg", z).double()
        m = m0 + (1 - b1) * (g - m0)
        v = b2 * state.get("exp_avg_sq", z).double() + (1 - b2) * g * g
        new["exp_avg"], new["exp_avg_sq"] = m, v
        p = p - (lr / (1 - b1 ** t)) * m / (v.sqrt() / math.sqrt(1 - b2 ** t) + eps)
    return p, new


SETTINGS = (
    [("sgd", dict(lr=1e-2, momentum=mu, nesterov=nv, weight_decay=wd))
     for mu in (0.0, 0.9, 0.99) for nv in (False, True) if not (nv and mu == 0) for wd in (0.0, 0.01)]
    + [(k, dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)) for k in ("adam", "adamw")
       for wd in (0.0, 0.01)]
    + [("adam", dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.1))]
    + [("rmsprop", dict(lr=1e-3, alpha=0.99, eps=1e-8, weight_decay=wd)) for wd in (0.0, 0.01)]
)
_TORCH = {"sgd": torch.optim.SGD, "adam": torch.optim.Adam, "adamw": torch.optim.AdamW,
          "rmsprop": torch.optim.RMSprop}


@pytest.mark.parametrize("kind,hp", SETTINGS, ids=lambda v: v if isinstance(v, str) else "-".join(
    f"{k}{x}" for k, x in v.items()))
def test_fp64_restatement_is_torch_optim(kind, hp):
    """3 steps of torch.optim on fp64 CPU tensors == ref_step to 1e-12 relative (parameters and states)."""
    gen = torch.Generator().manual_seed(3)
    p = torch.nn.Parameter(torch.randn(257, dtype=torch.float64, generator=gen))
    opt = _TORCH[kind]([p], **hp)
    rp, rstate = p.detach().clone(), {}
    for t in (1, 2, 3):
        g = torch.randn(257, dtype=torch.float64, generator=gen) * 10.0 ** float(t - 2)
        p.grad = g.clone()
        opt.step()
        rp, rstate = ref_step(kind, rp, rstate, g, t, **hp)
        torch.testing.assert_close(p.detach(), rp, rtol=1e-12, atol=0)
        for k, v in rstate.items():
            torch.testing.assert_close(opt.state[p][k], v, rtol=1e-12, atol=0)
        assert set(rstate) == set(opt.state[p]) - {"step"}


def test_clip_and_scale_enter_as_factors_of_the_gradient():
    """grad_scale and clip_coef multiply the gradient before the weight decay is added (clip_grad_norm_
    scales .grad, then optimizer.step() adds wd * p)."""
    gen = torch.Generator().manual_seed(4)
    p0 = torch.randn(64, dtype=torch.float64, generator=gen)
    g = torch.randn(64, dtype=torch.float64, generator=gen)
    hp = dict(lr=1e-2, momentum=0.9, weight_decay=0.01)
    p = torch.nn.Parameter(p0.clone())
    p.grad = g.clone()
    max_norm = 0.5 * float(g.norm())
    total = torch.nn.utils.clip_grad_norm_([p], max_norm)
    coef = min(1.0, max_norm / (float(total) + 1e-6))
    torch.optim.SGD([p], **hp).step()
    rp, _ = ref_step("sgd", p0, {}, g, 1, clip_coef=coef, **hp)
    torch.testing.assert_close(p.detach(), rp, rtol=1e-12, atol=0)


# -- flat buffers <-> state_dict -----------------------------------------------------------------
LAYOUT = [((2, 3), 8, False), ((4,), 0, False), ((3, 5), 16, True), ((5,), 32, False)]  # parameters() order
NPARAM = 40
GROUPS = {"rmsprop": dict(lr=1e-3, alpha=0.9), "sgd": dict(lr=1e-2, momentum=0.9), "adam": dict(lr=1e-3),
          "adamw": dict(lr=1e-3, weight_decay=0.02)}


@pytest.mark.parametrize("kind", ["rmsprop", "sgd", "adam", "adamw"])
def test_state_dict_conversion_round_trip_and_torch_loads_it(kind):
    group = fo.torch_defaults(kind, **GROUPS[kind])
    keys = fo.state_keys(kind, group)
    bufs = [torch.arange(NPARAM, dtype=torch.float32) + 100 * (j + 1) for j in range(len(keys))]
    sd = fo.flat_to_state_dict(kind, group, LAYOUT, bufs, 7)
    # torch's layout: indices in parameters() order, parameter-shaped tensors, per-parameter step, no state
    # for the no-gradient entry, a complete param_group
    params = [torch.nn.Parameter(torch.zeros(s)) for s, _, _ in LAYOUT]
    topt = _TORCH[kind](params, **GROUPS[kind])
    assert sd["param_groups"][0]["params"] == [0, 1, 2, 3]
    assert set(sd["param_groups"][0]) == set(topt.state_dict()["param_groups"][0])
    assert sorted(sd["state"]) == [0, 1, 3]
    for i, (shape, off, _) in enumerate(LAYOUT):
        if i == 2:
            continue
        st = sd["state"][i]
        assert set(st) == set(keys) | ({"step"} if kind != "sgd" else set())
        if kind != "sgd":
            assert st["step"].dtype == torch.float32 and float(st["step"]) == 7.0
        for j, k in enumerate(keys):
            assert tuple(st[k].shape) == shape
            assert torch.equal(st[k].reshape(-1), bufs[j][off:off + math.prod(shape)])
    topt.load_state_dict(sd)
    for i, p in enumerate(params):
        for k in keys:
            if i != 2:
                assert torch.equal(topt.state[p][k], sd["state"][i][k])
    assert params[2] not in topt.state or not topt.state[params[2]]
    # and back, from torch's own state_dict: the same flat buffers on the entries, zeros elsewhere
    back, step, g = fo.state_dict_to_flat(kind, topt.state_dict(), LAYOUT, NPARAM)
    assert step == (7 if kind != "sgd" else 1) and g["lr"] == GROUPS[kind]["lr"]
    mask = torch.zeros(NPARAM, dtype=torch.bool)
    for i, (shape, off, nograd) in enumerate(LAYOUT):
        if not nograd:
            mask[off:off + math.prod(shape)] = True
    for b, src in zip(back, bufs):
        assert torch.equal(b[mask], src[mask]) and float(b[~mask].abs().max()) == 0.0


def test_state_dict_before_the_first_step_is_empty_and_bad_dicts_are_refused():
    group = fo.torch_defaults("adam")
    sd = fo.flat_to_state_dict("adam", group, LAYOUT, [torch.zeros(NPARAM)] * 2, 0)
    assert sd["state"] == {}
    bufs, step, _ = fo.state_dict_to_flat("adam", sd, LAYOUT, NPARAM)
    assert step == 0 and all(float(b.abs().max()) == 0 for b in bufs)
    sd = fo.flat_to_state_dict("rmsprop", fo.torch_defaults("rmsprop"), LAYOUT, [torch.ones(NPARAM)], 2)
    with pytest.raises(ValueError):  # an RMSprop checkpoint into Adam
        fo.state_dict_to_flat("adam", sd, LAYOUT, NPARAM)
    with pytest.raises(ValueError):
        fo.state_dict_to_flat("rmsprop", sd, LAYOUT[:3], NPARAM)


# -- build_optimizer and the guards ---------------------------------------------------------------
def _config(kind):
    return SimpleNamespace(OPTIM=SimpleNamespace(TYPE=kind, LR=2e-3, MOMENTUM=0.95, WEIGHT_DECAY=0.02,
                                                 BETAS=[0.8, 0.9], EPS=1e-6),
                           LR_SCHEDULER=SimpleNamespace(TYPE=None))


@pytest.mark.parametrize("kind,cls", [("sgd", "SGD"), ("adam", "Adam"), ("adamw", "AdamW"), ("rmsprop", "RMSprop")])
def test_build_optimizer_returns_the_native_classes(kind, cls):
    import fall_multimodal_amd as f3
    model = torch.nn.Linear(3, 2)
    opt, sched = f3.build_optimizer(model, _config(kind))
    assert type(opt) is getattr(f3, cls) and sched is None
    assert isinstance(opt, torch.optim.Optimizer) and fo.optimizer_kind(opt) == kind
    g = opt.param_groups[0]
    assert g["lr"] == 2e-3
    if kind == "sgd":
        assert g["momentum"] == 0.95 and g["weight_decay"] == 0.02 and g["dampening"] == 0 and not g["nesterov"]
    elif kind != "rmsprop":
        assert tuple(g["betas"]) == (0.8, 0.9) and g["eps"] == 1e-6 and g["weight_decay"] == 0.02
    # torch's own param_group keys, so the state_dict layouts agree
    if kind != "rmsprop":
        ref = getattr(torch.optim, cls)(model.parameters(), lr=1e-3).param_groups[0]
        assert set(g) == set(ref)


def test_unsupported_settings_raise():
    import fall_multimodal_amd as f3
    ps = lambda: [torch.nn.Parameter(torch.zeros(4))]  # noqa: E731
    for make in (lambda: f3.SGD(ps(), lr=1e-2, momentum=0.9, dampening=0.1),
                 lambda: f3.SGD(ps(), lr=1e-2, maximize=True),
                 lambda: f3.Adam(ps(), amsgrad=True),
                 lambda: f3.AdamW(ps(), amsgrad=True),
                 lambda: f3.Adam(ps(), maximize=True),
                 lambda: f3.RMSprop(ps(), centered=True),
                 lambda: f3.RMSprop(ps(), momentum=0.9)):
        with pytest.raises(NotImplementedError):
            make()
    # a setting switched on after construction is caught at the step
    opt = f3.Adam(ps())
    opt.param_groups[0]["amsgrad"] = True
    opt.param_groups[0]["params"][0].grad = torch.zeros(4)
    with pytest.raises(NotImplementedError):
        opt.step()
    # torch's optimizers with such settings are refused by TrainStep's reading of them too
    t = torch.optim.SGD(ps(), lr=1e-2, momentum=0.9, dampening=0.5)
    with pytest.raises(NotImplementedError):
        fo.check_supported(fo.optimizer_kind(t), t.param_groups[0])
    assert f3.RMSprop(ps(), lr=1e-3).defaults == dict(lr=1e-3, alpha=0.99, eps=1e-8)  # weight_decay=0: as before
    assert f3.RMSprop(ps(), lr=1e-3, weight_decay=0.01).defaults["weight_decay"] == 0.01


def test_c_abi_refuses_unsupported_configs():
    """F3_EINVAL from f3_optim_step before anything touches the device (host-side validation)."""
    from fall_multimodal_amd import _lib, ops
    L = _lib.lib()
    dummy = torch.zeros(64)  # host memory: never dereferenced, the calls fail validation first
    base = dict(kind=_lib.OPT_ADAM, nesterov=False, lr=1e-3, alpha=0.99, eps=1e-8, momentum=0.0, beta1=0.9,
                beta2=0.999, weight_decay=0.0, max_norm=0.0, grad_scale=1.0)

    def status(**over):
        c = ops.optim_config(**{**base, **over})
        return L.f3_optim_step(c, _lib.ptr(dummy), _lib.ptr(dummy), _lib.ptr(dummy), _lib.ptr(dummy), 16,
                               _lib.ptr(dummy), None)

    assert status(kind=_lib.OPT_RMSPROP, momentum=0.9) == _lib.F3_EINVAL
    assert status(kind=_lib.OPT_SGD, nesterov=True) == _lib.F3_EINVAL
    assert status(kind=7) == _lib.F3_EINVAL
    assert status(beta1=1.0) == _lib.F3_EINVAL
    assert status(lr=float("nan")) == _lib.F3_EINVAL
    assert status(weight_decay=-1.0) == _lib.F3_EINVAL
    assert status(skip=(2, 4)) == _lib.F3_EINVAL  # not a multiple of 4
    assert int(L.f3_optim_scalars_bytes()) % 8 == 0 and int(L.f3_optim_scalars_bytes()) >= 24
