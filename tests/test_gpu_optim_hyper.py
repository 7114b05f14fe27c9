"""The optimizer's hyper-parameters as device values (needs an MI355X): f3_optim_hyper_set writes the block,
f3_optim_step_hyper's launches read it, and a captured TrainStep follows a scheduler on replay.

No tolerance anywhere: the device-reading kernels run the arithmetic of the by-value ones on the same
values (the same opt_update / rmsprop body, the OptArgs derived by the same expressions), so every
comparison is torch.equal against f3_optim_step / f3_rmsprop_step or against an eager TrainStep. bf16x3 is
used for the whole-step tests because its step is bit-deterministic (tests/test_gpu_determinism.py) and a
captured step already equals an eager one bit for bit (test_captured_adam_step_replays_bitwise)."""
import ctypes

import pytest
import torch

from oracle import model_cpu as oc
from oracle.prng import synthetic_batch

pytestmark = pytest.mark.gpu


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda")


def _keys(kind, hp):
    from fall_multimodal_amd import optim as fo
    return fo.state_keys(kind, hp)


def _cfg(kind, hp, max_norm, grad_scale, skip=()):
    from fall_multimodal_amd import ops, optim as fo
    return ops.optim_config(max_norm=max_norm, grad_scale=grad_scale, skip=skip, **fo.hyper(kind, hp))


def _legacy(kind, hp, max_norm):
    return kind == "rmsprop" and not hp.get("weight_decay", 0) and not max_norm


def _by_value(kind, hp, p, states, g, scalars, grad_scale, max_norm, skip):
    """f3_optim_step, or f3_rmsprop_step where the structure is plain RMSprop (what TrainStep's eager step issues)."""
    from fall_multimodal_amd import _lib
    s = list(states) + [None, None]
    if _legacy(kind, hp, max_norm):
        st = _lib.lib().f3_rmsprop_step(_lib.ptr(p), _lib.ptr(s[0]), _lib.ptr(g), p.numel(), hp["lr"], hp["alpha"],
                                        hp["eps"], grad_scale, _lib.stream_handle())
    else:
        st = _lib.lib().f3_optim_step(_cfg(kind, hp, max_norm, grad_scale, skip), _lib.ptr(p), _lib.ptr(s[0]),
                                      _lib.ptr(s[1]), _lib.ptr(g), p.numel(), _lib.ptr(scalars), _lib.stream_handle())
    _lib.check(st, f"{kind} step by value")


def _set(kind, hp, block, grad_scale, max_norm):
    from fall_multimodal_amd import _lib
    return _lib.lib().f3_optim_hyper_set(_cfg(kind, hp, max_norm, grad_scale), _lib.ptr(block), _lib.stream_handle())


def _from_block(kind, hp, p, states, g, block, scalars, max_norm, skip):
    """f3_optim_step_hyper with a configuration that carries the structure only: every value in it is a
    decoy, so a kernel that took one from the configuration would show."""
    from fall_multimodal_amd import _lib
    decoy = dict(hp, lr=0.7, weight_decay=0.3 if hp.get("weight_decay", 0) else 0.0)
    if "alpha" in hp:
        decoy.update(alpha=0.5, eps=0.25)
    if "betas" in hp:
        decoy.update(betas=(0.3, 0.4), eps=0.25)
    if hp.get("momentum", 0):
        decoy["momentum"] = 0.123
    cfg = _cfg(kind, decoy, 123.0 if max_norm else 0.0, 0.321, skip)
    s = list(states) + [None, None]
    st = _lib.lib().f3_optim_step_hyper(cfg, _lib.ptr(p), _lib.ptr(s[0]), _lib.ptr(s[1]), _lib.ptr(g), p.numel(),
                                        _lib.ptr(block), _lib.ptr(scalars), _lib.stream_handle())
    _lib.check(st, f"{kind} step from the block")


def _data(n, seed, d, steps=3):  # as tests/test_gpu_optim.py makes its buffers
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen).to(d)
    grads = [(torch.randn(n, generator=gen) * 10.0 ** float(k - 1)).to(d) for k in range(steps)]
    return p, grads


def _schedule(kind, hp, max_norm):
    """Three steps' (hp, max_norm): lr changes before each; before the second also eps, betas / alpha,
    the momentum, weight decay and max_norm, each within its structure (zero stays zero)."""
    out = []
    for k, f in enumerate((1.0, 0.5, 0.1)):
        h = dict(hp, lr=hp["lr"] * f)
        m = max_norm
        if k >= 1:
            if "eps" in h:
                h["eps"] = 1e-6
            if "alpha" in h:
                h["alpha"] = 0.9
            if "betas" in h:
                h["betas"] = (0.8, 0.99)
            if h.get("momentum", 0):
                h["momentum"] = 0.8
            if h.get("weight_decay", 0):
                h["weight_decay"] = 2.0 * h["weight_decay"]
            m = 0.5 * max_norm
        out.append((h, m))
    return out


SETTINGS = [
    ("rmsprop", dict(lr=1e-3, alpha=0.99, eps=1e-8)),
    ("rmsprop", dict(lr=1e-3, alpha=0.99, eps=1e-8, weight_decay=0.01)),
    ("sgd", dict(lr=1e-2, momentum=0.0, weight_decay=0.01)),
    ("sgd", dict(lr=1e-2, momentum=0.9, weight_decay=0.01)),
    ("sgd", dict(lr=1e-2, momentum=0.9, nesterov=True, weight_decay=0.01)),
    ("adam", dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)),
    ("adamw", dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)),
]
_ids = lambda v: v if isinstance(v, (str, int)) else "-".join(f"{k}{x}" for k, x in v.items())  # noqa: E731
# two skip ranges per n (floats, multiples of 4, inside n rounded up to 4); the last one covers the tail
SKIPS = {1: (0, 0, 0, 4), 5: (0, 0, 4, 4), 1023: (8, 16, 1020, 4), 4_194_304 + 7: (1024, 4096, 4_194_304, 8)}


# 1 / 5 / 1023: only a scalar tail, a tail after one float4, a tail of 3; 4_194_304 + 7 exceeds one pass of
# the capped grid (4096 x 256 x 4), one float more than tests/test_gpu_optim.py's flat test
@pytest.mark.parametrize("n", sorted(SKIPS), ids=_ids)
@pytest.mark.parametrize("kind,hp", SETTINGS, ids=_ids)
def test_block_form_equals_by_value_form_bitwise(kind, hp, n):
    """1. Three steps with the values changed before each: hyper_set + step_hyper on one set of buffers,
    the by-value call with the same per-step values on a twin set; parameters, states and step scalars
    bit-equal, gradients untouched. With and without clipping, grad_scale 1 and 0.5, with and without skip
    ranges."""
    d = dev()
    from fall_multimodal_amd import ops
    p_init, grads = _data(n, 300 + n % 89, d)
    kept = [g.clone() for g in grads]
    norm0 = float(torch.linalg.vector_norm(grads[0].double()))
    keys = _keys(kind, hp)
    for grad_scale in (1.0, 0.5):
        for max_norm in (0.0, 0.25 * norm0 * grad_scale):
            for skip in ((), SKIPS[n]):
                pa, pb = p_init.clone(), p_init.clone()
                sa = {k: torch.full((n,), 0.125, device=d) for k in keys}
                sb = {k: v.clone() for k, v in sa.items()}
                sca, scb, block = ops.optim_scalars(d), ops.optim_scalars(d), ops.optim_hyper(d)
                what = f"{kind} n={n} scale={grad_scale} max_norm={max_norm} skip={skip}"
                for (h, m), g in zip(_schedule(kind, hp, max_norm), grads):
                    assert _set(kind, h, block, grad_scale, m) == 0
                    _from_block(kind, h, pa, list(sa.values()), g, block, sca, m, skip)
                    _by_value(kind, h, pb, list(sb.values()), g, scb, grad_scale, m, skip)
                torch.cuda.synchronize()
                assert torch.equal(pa, pb), what
                if not skip:
                    assert not torch.equal(pa, p_init), what
                for k in keys:
                    assert torch.equal(sa[k], sb[k]), (what, k)
                if not _legacy(kind, hp, max_norm):  # t, bc1, bc2s, clip_coef, grad_norm
                    assert torch.equal(sca[:6].view(torch.int32), scb[:6].view(torch.int32)), what
                    assert int(ops.scalar_views(sca)[0].item()) == 3
                    if max_norm:
                        assert float(ops.scalar_views(sca)[3].item()) < 1.0, what  # it clipped
                else:
                    assert not bool(sca.any())  # as f3_rmsprop_step: no scalars touched
                got = ops.hyper_views(block).cpu().tolist()
                h, m = _schedule(kind, hp, max_norm)[-1]
                assert got[0] == h["lr"] and got[7] == m and got[8] == grad_scale
    for g, g0 in zip(grads, kept):
        assert torch.equal(g, g0)


@pytest.mark.parametrize("kind,hp,clip", [("adam", SETTINGS[5][1], True), ("rmsprop", SETTINGS[0][1], False)],
                         ids=["adam-clipped", "plain-rmsprop"])
def test_recorded_step_follows_the_block(kind, hp, clip):
    """2. f3_optim_step_hyper alone in a graph on raw buffers, replayed three times with f3_optim_hyper_set
    between the replays == three by-value eager steps, bit for bit."""
    d = dev()
    from fall_multimodal_amd import ops
    n = 3 * 1024 + 7
    p_init, grads = _data(n, 17, d)
    max_norm = 0.25 * float(torch.linalg.vector_norm(grads[0].double())) if clip else 0.0
    keys = _keys(kind, hp)
    pa, pb = p_init.clone(), p_init.clone()
    sa = {k: torch.zeros(n, device=d) for k in keys}
    sb = {k: torch.zeros(n, device=d) for k in keys}
    sca, scb, block = ops.optim_scalars(d), ops.optim_scalars(d), ops.optim_hyper(d)
    g_static = torch.zeros(n, device=d)
    sched = _schedule(kind, hp, max_norm)
    assert _set(kind, sched[0][0], block, 1.0, sched[0][1]) == 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _from_block(kind, hp, pa, list(sa.values()), g_static, block, sca, max_norm, ())
    torch.cuda.synchronize()
    assert torch.equal(pa, p_init)  # recorded, not run
    for (h, m), g in zip(sched, grads):
        g_static.copy_(g)
        assert _set(kind, h, block, 1.0, m) == 0
        graph.replay()
        _by_value(kind, h, pb, list(sb.values()), g, scb, 1.0, m, ())
    torch.cuda.synchronize()
    assert torch.equal(pa, pb) and not torch.equal(pa, p_init)
    for k in keys:
        assert torch.equal(sa[k], sb[k])
    if clip:
        assert torch.equal(sca[:6].view(torch.int32), scb[:6].view(torch.int32))
        assert int(ops.scalar_views(sca)[0].item()) == 3 and float(ops.scalar_views(sca)[3].item()) < 1.0


def test_hyper_set_validates_and_leaves_the_block():
    """3. F3_EINVAL for a negative lr, beta1 = 1, a NaN eps, grad_scale = 0, RMSprop momentum, a NULL block and
    a block at an address that is no multiple of 8; the block keeps the values of the last good call."""
    d = dev()
    from fall_multimodal_amd import _lib, ops
    adam = SETTINGS[5][1]
    block = ops.optim_hyper(d)
    assert block.numel() * 8 == _lib.lib().f3_optim_hyper_bytes() and not bool(block.any())
    assert _set("adam", adam, block, 0.5, 2.0) == 0
    torch.cuda.synchronize()
    good = ops.hyper_views(block).clone()
    assert good.cpu().tolist() == [1e-3, 0.99, 1e-8, 0.0, 0.9, 0.999, 0.01, 2.0, 0.5]
    bad = [("adam", dict(adam, lr=-1e-3), 1.0), ("adam", dict(adam, betas=(1.0, 0.999)), 1.0),
           ("adam", dict(adam, eps=float("nan")), 1.0), ("adam", adam, 0.0), ("adam", dict(adam, lr=float("inf")), 1.0),
           ("rmsprop", dict(lr=1e-3, alpha=1.0, eps=1e-8), 1.0)]
    for kind, hp, scale in bad:
        assert _set(kind, hp, block, scale, 2.0) == _lib.F3_EINVAL, (kind, hp, scale)
    cfg = _cfg("rmsprop", dict(lr=1e-3, alpha=0.99, eps=1e-8), 0.0, 1.0)
    cfg.momentum = 0.9  # RMSprop momentum: not built
    assert _lib.lib().f3_optim_hyper_set(cfg, _lib.ptr(block), _lib.stream_handle()) == _lib.F3_EINVAL
    ok = _cfg("adam", adam, 0.0, 1.0)
    assert _lib.lib().f3_optim_hyper_set(ok, None, _lib.stream_handle()) == _lib.F3_EINVAL
    odd = ctypes.c_void_p(block.data_ptr() + 4)
    assert _lib.lib().f3_optim_hyper_set(ok, odd, _lib.stream_handle()) == _lib.F3_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(ops.hyper_views(block), good)


# -- the whole step (the model, batch and helpers of tests/test_gpu_optim.py's step tests) -----------------
SPEC = oc.Spec(model="two_stgcan_bilstm", layout="coco_mmpose", num_class=11, sensor_dim=6)
B = 32
_STATE, _BATCH = {}, {}


def _init_state(seed):
    if seed not in _STATE:  # computed once, shared, never modified (load_state_dict copies)
        _STATE[seed] = oc.init_state(SPEC, seed)
    return _STATE[seed]


def _model(d, precision="bf16x3", seed=9):
    import fall_multimodal_amd as f3
    m = f3.TwoStreamSTGCAN_BiLSTM(3, {"layout": "coco_mmpose", "strategy": "spatial"}, 11, 6, device=d,
                                  precision=precision)
    m.load_state_dict(_init_state(seed))
    return m


def _batch(d, seed):
    if seed not in _BATCH:  # shared and read only: a captured step copies it into its static inputs
        _BATCH[seed] = tuple(torch.from_numpy(x).to(d) for x in synthetic_batch(B, 18, 11, 6, seed))
    return _BATCH[seed]


def _optimizer(kind, model, hp):
    import fall_multimodal_amd as f3
    return {"sgd": f3.SGD, "adam": f3.Adam, "adamw": f3.AdamW, "rmsprop": f3.RMSprop}[kind](model.parameters(), **hp)


def _twins(d, kind, hp, state=None, **step_kw):
    """(eager step, captured step) on twin models (loaded with `state` if given), each with its own optimizer."""
    import fall_multimodal_amd as f3
    out = []
    for captured in (False, True):
        model = _model(d)
        if state is not None:
            model.load_state_dict(state)
        step = f3.TrainStep(model, B, optimizer=_optimizer(kind, model, hp), **step_kw)
        if captured:
            sk, se, lb = (t.clone() for t in _batch(d, 40))
            step.capture(sk, se, step.prepare(sk, se, lb))
        out.append(step)
    return out


def _same_state(a, b, keys):
    assert torch.equal(a.model.flat_parameters(), b.model.flat_parameters())
    for k in keys:
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_captured_rmsprop_follows_per_update_schedule():
    """4. f3.RMSprop + CosineLRScheduler stepped per update (warm-up, then the cosine): five captured steps
    give the losses, parameters and square_avg of five eager steps. With the lr recorded by value the
    captured run kept the warm-up's first lr and this failed."""
    d = dev()
    from fall_multimodal_amd import ops
    from fall_multimodal_amd.optim import CosineLRScheduler
    eager, graph = _twins(d, "rmsprop", dict(lr=1e-3))
    losses = []
    for step in (eager, graph):
        sched = CosineLRScheduler(step.optimizer, t_initial=4, lr_min=1e-5, t_in_epochs=False, warmup_t=2,
                                     warmup_lr_init=1e-4)
        run, lrs = [], []
        for i in range(5):
            sched.step_update(i)
            lrs.append(step.optimizer.param_groups[0]["lr"])
            run.append(float(step(*_batch(d, 40 + i)).item()))
        assert len(set(lrs)) == 5  # the schedule moved before every step
        losses.append(run)
    torch.cuda.synchronize()
    print("eager", losses[0], "captured", losses[1])
    assert losses[0] == losses[1]
    _same_state(eager, graph, ["square_avg"])
    assert eager.steps_taken() == graph.steps_taken() == 5
    assert float(ops.hyper_views(graph.hyper)[0].item()) == 1e-5  # t = t_initial: lr_min


def test_captured_adamw_clipped_follows_per_epoch_schedule():
    """5. AdamW with weight decay and max_norm, two epochs of two steps with scheduler.step(e) between them."""
    d = dev()
    from fall_multimodal_amd.optim import CosineLRScheduler
    hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    eager, graph = _twins(d, "adamw", hp, max_norm=0.05)
    losses = []
    for step in (eager, graph):
        sched = CosineLRScheduler(step.optimizer, t_initial=4, lr_min=1e-5, t_in_epochs=True, warmup_t=1,
                                     warmup_lr_init=1e-4)
        run, lrs = [], []
        for e in range(2):
            sched.step(e)
            lrs.append(step.optimizer.param_groups[0]["lr"])
            for i in range(2):
                run.append(float(step(*_batch(d, 40 + 2 * e + i)).item()))
        assert lrs[0] == 1e-4 and 1e-4 < lrs[1] < 1e-3  # the warm-up value, then the cosine at t = 1
        losses.append(run)
    torch.cuda.synchronize()
    assert losses[0] == losses[1]
    _same_state(eager, graph, ["exp_avg", "exp_avg_sq", "step_count", "grad_norm", "clip_coef"])
    assert int(graph.step_count.item()) == 4 and float(graph.clip_coef.item()) < 1.0


def test_captured_accumulating_step_follows_lr():
    """6. accum_iter = 2, update=False / True calls, the lr changed between the updates."""
    d = dev()
    hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    eager, graph = _twins(d, "adam", hp, accum_iter=2)
    losses = []
    for step in (eager, graph):
        run = []
        for u, lr in enumerate((1e-3, 2.5e-4, 5e-5)):
            step.optimizer.param_groups[0]["lr"] = lr
            for i, update in enumerate((False, True)):
                run.append(float(step(*_batch(d, 40 + (2 * u + i) % 5), update=update).item()))
        losses.append(run)
    torch.cuda.synchronize()
    assert losses[0] == losses[1]
    _same_state(eager, graph, ["exp_avg", "exp_avg_sq", "step_count", "accum"])
    assert eager.steps_taken() == graph.steps_taken() == 3 and graph.pending == 0


def test_checkpoint_loaded_after_capture_is_followed():
    """7. load_optimizer_state_dict() of a checkpoint saved at another lr, after capture(): the next
    replays run at the loaded lr, as an eager twin loaded from the same checkpoint does."""
    d = dev()
    import fall_multimodal_amd as f3
    from fall_multimodal_amd import ops
    hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    donor_model = _model(d)
    donor = f3.TrainStep(donor_model, B, optimizer=_optimizer("adamw", donor_model, dict(hp, lr=3e-3)))
    for k in range(2):
        donor(*_batch(d, 40 + k))
    torch.cuda.synchronize()
    msd = {k: v.detach().clone() for k, v in donor_model.state_dict().items()}
    osd = donor.optimizer_state_dict()
    eager, graph = _twins(d, "adamw", hp, state=msd)
    for step in (eager, graph):
        step.load_optimizer_state_dict(osd)
        assert step.optimizer.param_groups[0]["lr"] == 3e-3
    losses = [[float(step(*_batch(d, 42 + k)).item()) for k in range(2)] for step in (eager, graph)]
    torch.cuda.synchronize()
    assert losses[0] == losses[1]
    _same_state(eager, graph, ["exp_avg", "exp_avg_sq", "step_count"])
    assert eager.steps_taken() == graph.steps_taken() == 4
    assert float(ops.hyper_views(graph.hyper)[0].item()) == 3e-3


def test_block_is_written_only_when_a_value_changed(monkeypatch):
    """8. capture() writes the block once; calls with nothing changed issue no write; a changed lr issues
    one; ops.hyper_views reads back the values in force."""
    d = dev()
    import fall_multimodal_amd as f3
    from fall_multimodal_amd import _lib, ops
    L = _lib.lib()
    real, calls = L.f3_optim_hyper_set, []

    def counted(*a):
        calls.append(1)
        return real(*a)

    monkeypatch.setattr(L, "f3_optim_hyper_set", counted)
    hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    model = _model(d)
    step = f3.TrainStep(model, B, optimizer=_optimizer("adamw", model, hp), max_norm=0.05)
    sk, se, lb = (t.clone() for t in _batch(d, 40))
    step.capture(sk, se, step.prepare(sk, se, lb))
    assert len(calls) == 1
    step(*_batch(d, 40))
    step(*_batch(d, 41))
    assert len(calls) == 1
    torch.cuda.synchronize()
    assert ops.hyper_views(step.hyper).cpu().tolist() == [1e-3, 0.99, 1e-8, 0.0, 0.9, 0.999, 0.01, 0.05, 1.0]
    step.optimizer.param_groups[0]["lr"] = 2e-4
    step.max_norm = 0.025
    step(*_batch(d, 42))
    step(*_batch(d, 43))
    assert len(calls) == 2
    torch.cuda.synchronize()
    assert ops.hyper_views(step.hyper).cpu().tolist() == [2e-4, 0.99, 1e-8, 0.0, 0.9, 0.999, 0.01, 0.025, 1.0]


@pytest.mark.parametrize("case", ["momentum", "weight_decay", "max_norm"])
def test_structure_change_after_capture_raises(case):
    """9. A change that needs other launches than the recorded ones raises ValueError at the next call and
    leaves the parameters as they were."""
    d = dev()
    import fall_multimodal_amd as f3
    kind, hp = {"momentum": ("sgd", dict(lr=1e-3, momentum=0.0)), "weight_decay": ("rmsprop", dict(lr=1e-3)),
                "max_norm": ("adam", dict(lr=1e-3))}[case]
    model = _model(d)
    step = f3.TrainStep(model, B, optimizer=_optimizer(kind, model, hp))
    sk, se, lb = (t.clone() for t in _batch(d, 40))
    step.capture(sk, se, step.prepare(sk, se, lb))
    step(*_batch(d, 40))
    torch.cuda.synchronize()
    before = model.flat_parameters().detach().clone()
    if case == "momentum":
        step.optimizer.param_groups[0]["momentum"] = 0.9
    elif case == "weight_decay":
        step.optimizer.param_groups[0]["weight_decay"] = 0.01
    else:
        step.max_norm = 1.0
    with pytest.raises(ValueError, match="capture"):
        step(*_batch(d, 41))
    torch.cuda.synchronize()
    assert torch.equal(model.flat_parameters(), before)
    assert step.steps_taken() == 1
