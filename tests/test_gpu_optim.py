"""The native SGD / Adam / AdamW / RMSprop-with-decay updates and the fixed-order gradient norm on
the GPU (needs an MI355X), against the fp64 restatement of torch.optim's arithmetic that
tests/test_optim_native.py pins to torch (ref_step).

Tolerances are the project's RMSprop gates (tests/test_gpu_parity.py): parameters rtol 1e-6 / atol 1e-7,
state tensors rtol 1e-5 / atol 1e-12. Every step is compared with the formulas applied to the state the
kernel started from (the pattern of test_backward_rmsprop_per_layer_updates), so the bound is one
step's rounding: the kernels evaluate the recurrences in fp64 and round once (<= 2^-24 relative on a
state), and the fp32 sqrt / division err by a few ulp of an update of at most ~lr (~1e-9 absolute).
The norm is an fp64 sum of exact squares rounded to fp32 once: rtol 2^-22."""
import numpy as np
import pytest
import torch

from oracle import model_cpu as oc
from oracle.prng import synthetic_batch
from test_optim_native import ref_step

pytestmark = pytest.mark.gpu

P_TOL = dict(rtol=1e-6, atol=1e-7)
S_TOL = dict(rtol=1e-5, atol=1e-12)
NORM_RTOL = 2.0 ** -22
K_RANGES = 8  # kRmsRanges (csrc/sensor.h)


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda")


def _launch(kind, hp, p, states, g, scalars, grad_scale=1.0, max_norm=0.0, skip=(), ranges=None):
    """f3_optim_step (or f3_optim_step_ranges) on torch tensors, in place."""
    import ctypes
    from fall_multimodal_amd import _lib, ops, optim as fo
    cfg = ops.optim_config(max_norm=max_norm, grad_scale=grad_scale, skip=skip, **fo.hyper(kind, hp))
    s = list(states) + [None, None]
    if ranges is None:
        st = _lib.lib().f3_optim_step(cfg, _lib.ptr(p), _lib.ptr(s[0]), _lib.ptr(s[1]), _lib.ptr(g), p.numel(),
                                      _lib.ptr(scalars), _lib.stream_handle())
    else:
        lo = (ctypes.c_int64 * len(ranges))(*[r[0] for r in ranges])
        ln = (ctypes.c_int64 * len(ranges))(*[r[1] for r in ranges])
        st = _lib.lib().f3_optim_step_ranges(cfg, _lib.ptr(p), _lib.ptr(s[0]), _lib.ptr(s[1]), _lib.ptr(g),
                                             len(ranges), lo, ln, _lib.ptr(scalars), _lib.stream_handle())
    _lib.check(st, f"{kind} step")


def _keys(kind, hp):
    from fall_multimodal_amd import optim as fo
    return fo.state_keys(kind, hp)


def _data(n, seed, d, steps=3):
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen).to(d)
    grads = [(torch.randn(n, generator=gen) * 10.0 ** float(k - 1)).to(d) for k in range(steps)]
    return p, grads


def _check_step(kind, hp, p0, st0, g, t, p, st, grad_scale=1.0, clip_coef=1.0, what=""):
    """p / st after one step == the fp64 formulas from (p0, st0); returns the worst differences."""
    rp, rst = ref_step(kind, p0, st0, g, t, grad_scale=grad_scale, clip_coef=clip_coef, **hp)
    worst = {"param": float((p.double() - rp).abs().max())}
    for k, v in rst.items():
        worst[k] = float(((st[k].double() - v).abs() / v.abs().clamp_min(1e-30)).max())
    print(f"{kind} {what} t={t} worst |dp|={worst['param']:.3e} "
          + " ".join(f"rel {k}={worst[k]:.3e}" for k in rst))
    for k, v in rst.items():
        torch.testing.assert_close(st[k].double(), v, **S_TOL)
    torch.testing.assert_close(p.double(), rp, **P_TOL)
    return worst


FLAT_SETTINGS = (
    [("sgd", dict(lr=1e-2, momentum=mu, nesterov=nv, weight_decay=wd))
     for mu in (0.0, 0.9, 0.99) for nv in (False, True) if not (nv and mu == 0) for wd in (0.0, 0.01)]
    + [(k, dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)) for k in ("adam", "adamw")
       for wd in (0.0, 0.01)]
    + [("rmsprop", dict(lr=1e-3, alpha=0.99, eps=1e-8, weight_decay=0.01))]
)
_ids = lambda v: v if isinstance(v, (str, int)) else "-".join(f"{k}{x}" for k, x in v.items())  # noqa: E731


# 4_194_304 + 7 exceeds one pass of the capped grid (4096 x 256 x 4): the stride loop and the scalar tail
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4_194_304 + 7], ids=_ids)
@pytest.mark.parametrize("kind,hp", FLAT_SETTINGS, ids=_ids)
def test_flat_kernel_against_fp64(kind, hp, n):
    """1. Three steps (Adam t = 1..3) of the flat kernel on synthetic gradients, grad_scale 1 and 0.5."""
    d = dev()
    from fall_multimodal_amd import ops
    for grad_scale in (1.0, 0.5):
        p, grads = _data(n, 100 + n % 97, d)
        st = {k: torch.zeros(n, device=d) for k in _keys(kind, hp)}
        scalars = ops.optim_scalars(d)
        for t, g in enumerate(grads, 1):
            p0, st0, g0 = p.clone(), {k: v.clone() for k, v in st.items()}, g.clone()
            _launch(kind, hp, p, list(st.values()), g, scalars, grad_scale=grad_scale)
            torch.cuda.synchronize()
            _check_step(kind, hp, p0, st0, g, t, p, st, grad_scale=grad_scale, what=f"n={n} scale={grad_scale}")
            assert torch.equal(g, g0)  # the gradient buffer is left as it was
            assert int(ops.scalar_views(scalars)[0].item()) == t
            assert float(ops.scalar_views(scalars)[3].item()) == 1.0  # clip_coef with clipping off


RANGE_KINDS = [("sgd", dict(lr=1e-2, momentum=0.0, weight_decay=0.01)),
               ("sgd", dict(lr=1e-2, momentum=0.9, nesterov=True, weight_decay=0.01)),
               ("adam", dict(lr=1e-3, weight_decay=0.01)), ("adamw", dict(lr=1e-3, weight_decay=0.01)),
               ("rmsprop", dict(lr=1e-3, weight_decay=0.01))]


@pytest.mark.parametrize("nranges", [1, K_RANGES])
@pytest.mark.parametrize("kind,hp", RANGE_KINDS, ids=_ids)
def test_ranges_kernel_matches_flat_bitwise(kind, hp, nranges):
    """2. The ranges shape (the per-layer updates inside the backward): unequal lengths, all multiples
    of 4, gaps between them. On its own elements it gives the flat kernel's bits (same build); every
    element in a gap is bit-unchanged, in the parameters and in the states."""
    d = dev()
    from fall_multimodal_amd import ops
    lens = [1028, 4, 8, 2052, 12, 516, 4, 260][:nranges]   # > one 256-thread workgroup's 1024 floats in places
    gaps = [4, 8, 4, 12, 4, 8, 4, 16][:nranges]
    ranges, off = [], 0
    for ln, gp in zip(lens, gaps):
        off += gp
        ranges.append((off, ln))
        off += ln
    n = off + 8
    inside = torch.zeros(n, dtype=torch.bool, device=d)
    for lo, ln in ranges:
        inside[lo:lo + ln] = True
    p_init, grads = _data(n, 7 + nranges, d, steps=2)
    pf, pr = p_init.clone(), p_init.clone()
    keys = _keys(kind, hp)
    sf = {k: torch.full((n,), 0.25, device=d) for k in keys}
    sr = {k: v.clone() for k, v in sf.items()}
    scf, scr = ops.optim_scalars(d), ops.optim_scalars(d)
    for g in grads:
        _launch(kind, hp, pf, list(sf.values()), g, scf)
        _launch(kind, hp, pr, list(sr.values()), g, scr, ranges=ranges)
    torch.cuda.synchronize()
    assert torch.equal(pr[inside], pf[inside]) and not torch.equal(pr[inside], p_init[inside])
    assert torch.equal(pr[~inside], p_init[~inside])
    for k in keys:
        assert torch.equal(sr[k][inside], sf[k][inside])
        assert bool((sr[k][~inside] == 0.25).all())
    assert int(ops.scalar_views(scr)[0].item()) == 2


@pytest.mark.parametrize("n", [5, 1023, 4_194_304 + 7])
def test_rmsprop_kind_is_rmsprop_step_bitwise(n):
    """3. f3_optim_step with kind RMSprop, no decay, no clipping == f3_rmsprop_step on the same inputs,
    bit for bit (parameters and square_avg). The one test here that also holds without the new kernels'
    arithmetic: it pins that the default path's bits did not move."""
    d = dev()
    from fall_multimodal_amd import _lib, ops
    hp = dict(lr=1e-3, alpha=0.99, eps=1e-8)
    p, grads = _data(n, 5, d)
    pa, pb = p.clone(), p.clone()
    sa, sb = torch.zeros(n, device=d), torch.zeros(n, device=d)
    scalars = ops.optim_scalars(d)
    for g in grads:
        for scale in (1.0, 0.5):
            _launch("rmsprop", hp, pa, [sa], g, scalars, grad_scale=scale)
            _lib.check(_lib.lib().f3_rmsprop_step(_lib.ptr(pb), _lib.ptr(sb), _lib.ptr(g), n, 1e-3, 0.99, 1e-8, scale,
                                                  _lib.stream_handle()), "rmsprop")
    torch.cuda.synchronize()
    assert torch.equal(pa, pb) and torch.equal(sa, sb)


def _norm_case(n, seed, d):
    gen = torch.Generator().manual_seed(seed)
    if seed == 0:
        return torch.zeros(n, device=d)
    if seed == 1:  # magnitudes spanning 1e-20 .. 1e3: the small squares underflow fp32, not fp64
        e = torch.rand(n, generator=gen, dtype=torch.float64) * 23.0 - 20.0
        return (torch.randn(n, generator=gen, dtype=torch.float64).sign() * 10.0 ** e).float().to(d)
    return torch.randn(n, generator=gen).to(d)


@pytest.mark.parametrize("n", [1, 5, 4097, 4_298_291])
@pytest.mark.parametrize("seed", [0, 1, 2], ids=["zeros", "wide", "randn"])
def test_grad_norm_fixed_order(n, seed):
    """4. The norm against torch.linalg.vector_norm in fp64 at rtol 2^-22 (fp64 sums of exact squares over
    <= 4.3 M elements err by well under 1e-9; the rest is the one rounding to fp32), bit-identical between
    two runs, and the clip coefficient min(1, max_norm / (norm + 1e-6))."""
    d = dev()
    from fall_multimodal_amd import ops
    g = _norm_case(n, seed, d)
    ref = float(torch.linalg.vector_norm(g.double()))
    hp = dict(lr=1e-2, momentum=0.9, weight_decay=0.01)
    runs = []
    for _ in range(2):
        p = torch.ones(n, device=d)
        buf = torch.zeros(n, device=d)
        sc = ops.optim_scalars(d)
        _launch("sgd", hp, p, [buf], g, sc, max_norm=0.5 * ref if ref else 1.0)
        torch.cuda.synchronize()
        runs.append((sc.clone(), p, buf))
    # (as integers: the block's fp64 partial sums, read as fp32 halves, can be NaN patterns)
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    _, _, _, coef, norm = ops.scalar_views(runs[0][0])
    norm, coef = float(norm.item()), float(coef.item())
    print(f"n={n} {seed}: norm {norm!r} fp64 {ref!r} rel {abs(norm - ref) / ref if ref else 0.0:.3e} coef {coef!r}")
    if ref == 0.0:
        assert norm == 0.0 and coef == 1.0
    else:
        assert abs(norm - ref) <= NORM_RTOL * ref
        want = min(1.0, 0.5 * ref / (ref + 1e-6))
        assert abs(coef - want) <= NORM_RTOL * want
    # grad_scale scales the norm (the gradient that is clipped is grad_scale * grads)
    sc = ops.optim_scalars(d)
    _launch("sgd", hp, torch.ones(n, device=d), [torch.zeros(n, device=d)], g, sc, max_norm=1.0, grad_scale=0.5)
    assert abs(float(ops.scalar_views(sc)[4].item()) - 0.5 * ref) <= NORM_RTOL * 0.5 * ref


@pytest.mark.parametrize("kind,hp", RANGE_KINDS, ids=_ids)
def test_clipped_update(kind, hp):
    """4 (cont.). max_norm below the norm: the update is the fp64 formula on clip_coef * grad (the
    coefficient the device holds), and the gradient buffer stays unscaled. max_norm above the norm: the
    same bits as clipping off."""
    d = dev()
    from fall_multimodal_amd import ops
    n = 4097
    p_init, grads = _data(n, 21, d, steps=2)
    keys = _keys(kind, hp)
    ref = float(torch.linalg.vector_norm(grads[0].double()))
    # below the norm
    p, st, sc = p_init.clone(), {k: torch.zeros(n, device=d) for k in keys}, ops.optim_scalars(d)
    for t, g in enumerate(grads, 1):
        p0, st0, g0 = p.clone(), {k: v.clone() for k, v in st.items()}, g.clone()
        _launch(kind, hp, p, list(st.values()), g, sc, max_norm=0.25 * ref)
        torch.cuda.synchronize()
        coef = float(ops.scalar_views(sc)[3].item())
        norm = float(torch.linalg.vector_norm(g.double()))
        want = min(1.0, 0.25 * ref / (norm + 1e-6))
        assert coef < 1.0 and abs(coef - want) <= NORM_RTOL * want
        _check_step(kind, hp, p0, st0, g, t, p, st, clip_coef=coef, what="clipped")
        assert torch.equal(g, g0)
    # above the norm == off
    outs = []
    for max_norm in (0.0, 1e4 * ref):
        p, st, sc = p_init.clone(), {k: torch.zeros(n, device=d) for k in keys}, ops.optim_scalars(d)
        for g in grads:
            _launch(kind, hp, p, list(st.values()), g, sc, max_norm=max_norm)
        torch.cuda.synchronize()
        outs.append((p, st, float(ops.scalar_views(sc)[3].item())))
    assert outs[0][2] == 1.0 and outs[1][2] == 1.0
    assert torch.equal(outs[0][0], outs[1][0])
    for k in keys:
        assert torch.equal(outs[0][1][k], outs[1][1][k])


# -- the whole step ------------------------------------------------------------------------------
SPEC = oc.Spec(model="two_stgcan_bilstm", layout="coco_mmpose", num_class=11, sensor_dim=6)
B = 32
STEP_KINDS = {"sgd": dict(lr=1e-3, momentum=0.9, weight_decay=0.01),
              "adam": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01),
              "adamw": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)}
_STATE = {}


def _init_state(seed):
    if seed not in _STATE:  # computed once, shared, never modified (load_state_dict copies)
        _STATE[seed] = oc.init_state(SPEC, seed)
    return _STATE[seed]


def _model(d, precision, seed=9):
    import fall_multimodal_amd as f3
    m = f3.TwoStreamSTGCAN_BiLSTM(3, {"layout": "coco_mmpose", "strategy": "spatial"}, 11, 6, device=d,
                                  precision=precision)
    m.load_state_dict(_init_state(seed))
    return m


def _batch(d, seed):
    return tuple(torch.from_numpy(x).to(d) for x in synthetic_batch(B, 18, 11, 6, seed))


def _optimizer(kind, model, hp):
    import fall_multimodal_amd as f3
    return {"sgd": f3.SGD, "adam": f3.Adam, "adamw": f3.AdamW, "rmsprop": f3.RMSprop}[kind](model.parameters(), **hp)


@pytest.mark.parametrize("mode", ["per_layer", "phased", "clipped"])
@pytest.mark.parametrize("kind", ["sgd", "adam", "adamw"])
@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_whole_step_matches_fp64_formulas(precision, kind, mode):
    """5. Two TrainStep steps with f3.SGD / Adam / AdamW: after each, the parameters and the state buffers
    equal the fp64 formulas applied to the step's own gradients (step.grads) and the previous state - every
    parameter updated exactly once. per_layer: f3_net_backward_optim's updates on the queues that finish
    each layer; phased: the flat f3_optim_step after the two-phase backward; clipped: max_norm = half of
    the first step's norm (one flat update after the join)."""
    d = dev()
    import fall_multimodal_amd as f3
    hp = STEP_KINDS[kind]
    model = _model(d, precision)
    opt = _optimizer(kind, model, hp)
    step = f3.TrainStep(model, B, optimizer=opt, phased=(mode == "phased"))
    assert step.kind == kind and step.fused_optimizer and step.phased == (mode == "phased")
    assert lib_fused(model) == 1
    if mode == "clipped":
        sk, se, lb = _batch(d, 40)
        step.forward_backward(sk, se, step.prepare(sk, se, lb))  # the first step's gradients, no update
        torch.cuda.synchronize()
        step.max_norm = 0.5 * float(torch.linalg.vector_norm(step.grads.double()))
    keys = _keys(kind, hp)
    for k in range(2):
        sk, se, lb = _batch(d, 40 + k)
        p0 = model.flat_parameters().detach().clone()
        st0 = {key: getattr(step, key).clone() for key in keys}
        step(sk, se, lb)
        torch.cuda.synchronize()
        g = step.grads
        coef = float(step.clip_coef.item())
        if mode == "clipped":
            norm = float(torch.linalg.vector_norm(g.double()))
            assert abs(float(step.grad_norm.item()) - norm) <= NORM_RTOL * norm
            want = min(1.0, step.max_norm / (norm + 1e-6))
            assert abs(coef - want) <= NORM_RTOL * want
            if k == 0:
                assert 0.45 < coef < 0.55, coef
        else:
            assert coef == 1.0
        _check_step(kind, hp, p0, st0, g, k + 1, model.flat_parameters().detach(),
                    {key: getattr(step, key) for key in keys}, clip_coef=coef, what=f"{precision} {mode}")
        assert int(step.step_count.item()) == k + 1 and step.steps_taken() == k + 1


def lib_fused(model):
    from fall_multimodal_amd import _lib
    return _lib.lib().f3_net_fused_rmsprop(model._native.h)


@pytest.mark.parametrize("mode", ["per_layer", "flat"])
@pytest.mark.parametrize("kind,hp", [("adamw", dict(lr=1e-3, weight_decay=0.01)),
                                     ("sgd", dict(lr=1e-3, momentum=0.9, weight_decay=0.01))], ids=_ids)
def test_no_gradient_entries_are_left_alone(kind, hp, mode):
    """6. The UR 3-stream model (CNN1D sensor branch, V=14): its cnn.fc.weight / cnn.fc.bias never receive
    a gradient (the forward does not use them; .grad stays None in the reference), so an update with weight
    decay must not touch them, nor the 16-byte pads of the flat buffer; every other entry moves."""
    d = dev()
    import fall_multimodal_amd as f3
    spec = oc.Spec(model="two_stgcan_bilstm", layout="coco_cut", num_class=2, sensor="cnn_bilstm", sensor_dim=4,
                   sensor_classes=2, softmax_output=True, naming="notebook")
    model = f3.TwoStreamSpatialTemporalGraph({"layout": "coco_cut", "strategy": spec.strategy}, 2, sensor="cnn_bilstm",
                                             sensor_dim=4, sensor_classes=2, device=d, precision="bf16x3")
    model.load_state_dict(oc.init_state(spec, 5))
    step = f3.TrainStep(model, B, optimizer=_optimizer(kind, model, hp), phased=(mode == "flat"))
    nograd = sorted(step._nograd)
    assert len(nograd) == 2 and nograd[0].endswith("fc.bias") and nograd[1].endswith("fc.weight"), nograd
    assert all(".cnn." in n or n.startswith("cnn.") for n in nograd), nograd
    sk, se, lb = (torch.from_numpy(x).to(d) for x in synthetic_batch(B, 14, 2, 4, 3))
    flat = model.flat_parameters()
    before = flat.detach().clone()
    step(sk, se, lb)
    torch.cuda.synchronize()
    after = flat.detach()
    covered = torch.zeros(flat.numel(), dtype=torch.bool, device=d)
    for name, shape, off in model.param_views():
        n = int(np.prod(shape))
        covered[off:off + n] = True
        same = torch.equal(after[off:off + n].view(torch.int32), before[off:off + n].view(torch.int32))
        assert same == (name in step._nograd), name
        for key in _keys(kind, hp):  # no state either
            if name in step._nograd:
                assert not bool(getattr(step, key)[off:off + n].any()), (name, key)
    assert int((~covered).sum()) > 0  # the layout has pads
    assert torch.equal(after[~covered].view(torch.int32), before[~covered].view(torch.int32))
    for key in _keys(kind, hp):
        assert not bool(getattr(step, key)[~covered].any())
    # and the state_dict carries no state for them
    sd = step.optimizer_state_dict()
    names = [n for n, _ in model.named_parameters()]
    assert sorted(names[i] for i in range(len(names)) if i not in sd["state"]) == nograd


def test_captured_adam_step_replays_bitwise():
    """7. bf16x3 + Adam captured into HIP graphs: three replays give the losses of three eager steps of a
    twin model, bit for bit (tests/test_gpu_graph.py does this for RMSprop), and the device step count
    reads 3 + the capture's own warm-up count, which is 0: capture() warms up with forward + backward
    only, and the optimizer launches inside the capture are recorded, not run."""
    d = dev()
    import fall_multimodal_amd as f3
    hp = STEP_KINDS["adam"]
    sk, se, lb = _batch(d, 62)
    model = _model(d, "bf16x3", seed=61)
    step = f3.TrainStep(model, B, optimizer=_optimizer("adam", model, hp))
    lbl = step.prepare(sk, se, lb)
    step.capture(sk, se, lbl)
    torch.cuda.synchronize()
    assert int(step.step_count.item()) == 0
    losses = [float(step(sk, se, lbl).item()) for _ in range(3)]
    assert int(step.step_count.item()) == 3 and step.steps_taken() == 3
    twin = _model(d, "bf16x3", seed=61)
    tstep = f3.TrainStep(twin, B, optimizer=_optimizer("adam", twin, hp))
    ref = [float(tstep(sk, se, lb).item()) for _ in range(3)]
    assert all(np.isfinite(losses)) and losses == ref, (losses, ref)
    assert torch.equal(model.flat_parameters(), twin.flat_parameters())
    assert torch.equal(step.exp_avg, tstep.exp_avg) and torch.equal(step.exp_avg_sq, tstep.exp_avg_sq)


@pytest.mark.parametrize("kind,hp", [("adamw", STEP_KINDS["adamw"]), ("rmsprop", dict(lr=1e-3))], ids=_ids)
def test_checkpoint_round_trip(kind, hp):
    """8. Two steps, save model.state_dict() + step.optimizer_state_dict(), load both into a fresh model and
    step: a third step on each gives bit-identical parameters (bf16x3). The saved dict also loads into
    torch.optim's optimizer over the model's parameters, with equal tensors. RMSprop (the default path, whose
    square_avg the reference's checkpoint line would otherwise lose) included."""
    d = dev()
    import fall_multimodal_amd as f3
    model = _model(d, "bf16x3")
    step = f3.TrainStep(model, B, optimizer=_optimizer(kind, model, hp))
    for k in range(2):
        step(*_batch(d, 40 + k))
    torch.cuda.synchronize()
    msd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    osd = step.optimizer_state_dict()
    assert step.steps_taken() == 2
    # a fresh model and step
    model2 = _model(d, "bf16x3", seed=10)
    model2.load_state_dict(msd)
    step2 = f3.TrainStep(model2, B, optimizer=_optimizer(kind, model2, dict(hp, lr=7e-3)))
    step2.load_optimizer_state_dict(osd)
    assert step2.steps_taken() == 2 and step2.optimizer.param_groups[0]["lr"] == hp["lr"]
    b3 = _batch(d, 42)
    step(*b3)
    step2(*b3)
    torch.cuda.synchronize()
    assert torch.equal(model.flat_parameters(), model2.flat_parameters())
    # torch's optimizer takes the same dict
    tcls = {"adamw": torch.optim.AdamW, "rmsprop": torch.optim.RMSprop}[kind]
    topt = tcls(model.parameters(), lr=5e-2)
    topt.load_state_dict(osd)
    assert topt.param_groups[0]["lr"] == hp["lr"]
    names = [n for n, _ in model.named_parameters()]
    assert sorted(osd["state"]) == list(range(len(names)))
    for i, p in enumerate(model.parameters()):
        for key, v in osd["state"][i].items():
            got = topt.state[p][key]
            assert got.shape == v.shape and torch.equal(got.cpu().float(), v.cpu().float()), (names[i], key)
            if key != "step":
                assert v.shape == p.shape
        assert float(osd["state"][i]["step"]) == 2.0
    # and back: torch's own state_dict loads into a step, giving the buffers that were saved
    from fall_multimodal_amd import optim as fo
    m3 = _model(d, "bf16x3")
    step3 = f3.TrainStep(m3, B, optimizer=_optimizer(kind, m3, hp))
    step3.load_optimizer_state_dict(topt.state_dict())
    saved, nsteps, _ = fo.state_dict_to_flat(kind, osd, step._layout(), step.grads.numel(), device=d)
    assert nsteps == 2 and step3.steps_taken() == 2
    for key, buf in zip(_keys(kind, hp), saved):
        assert torch.equal(getattr(step3, key), buf) and bool(buf.any())


@pytest.mark.parametrize("mode", ["flat", "per_tensor"])
@pytest.mark.parametrize("kind,hp", [("sgd", dict(lr=1e-3, momentum=0.9, nesterov=True, weight_decay=0.01)),
                                     ("adam", STEP_KINDS["adam"]), ("adamw", STEP_KINDS["adamw"]),
                                     ("rmsprop", dict(lr=1e-3, weight_decay=0.01))], ids=_ids)
def test_optimizer_classes_after_autograd_backward(kind, hp, mode):
    """The reference's own loop (model/main.py:112-127): loss.backward(); optimizer.step() with f3.SGD / Adam /
    AdamW / RMSprop(weight_decay). Over 3 steps every parameter and state tensor equals the fp64 formulas applied
    to its .grad and its previous state, on the one-launch flat path and on the per-tensor path (states in
    storage of their own, as after load_state_dict); the state_dict then loads into torch's optimizer."""
    d = dev()
    B8 = 8
    batch = [torch.from_numpy(x).to(d) for x in synthetic_batch(B8, 18, 11, 6, 17)]
    model = _model(d, "bf16x3", seed=5)
    params = list(model.parameters())
    opt = _optimizer(kind, model, hp)
    keys = _keys(kind, hp)
    if mode == "per_tensor":
        for p in params:
            for key in keys:
                opt.state[p][key] = torch.zeros_like(p)
            if kind != "sgd":
                opt.state[p]["step"] = torch.zeros((), dtype=torch.float32)
    for t in (1, 2, 3):
        opt.zero_grad()
        torch.nn.CrossEntropyLoss()(model(batch[0], batch[1]), batch[2]).backward()
        assert (opt._flat(opt.param_groups[0]) is not None) == (mode == "flat"), mode
        p0 = [p.detach().clone() for p in params]
        s0 = [{key: opt.state[p][key].clone() for key in keys if key in opt.state[p]} for p in params]
        opt.step()
        torch.cuda.synchronize()
        for p, a, b in zip(params, p0, s0):
            rp, rst = ref_step(kind, a, b, p.grad, t, **hp)
            torch.testing.assert_close(p.detach().double(), rp, **P_TOL)
            for key, v in rst.items():
                torch.testing.assert_close(opt.state[p][key].double(), v, **S_TOL)
    if kind != "sgd":
        assert all(int(opt.state[p]["step"]) == 3 for p in params)
    tcls = {"sgd": torch.optim.SGD, "adam": torch.optim.Adam, "adamw": torch.optim.AdamW,
            "rmsprop": torch.optim.RMSprop}[kind]
    topt = tcls(params, lr=1.0)
    topt.load_state_dict(opt.state_dict())
    assert topt.param_groups[0]["lr"] == hp["lr"]
    for p in params:
        for key in keys:
            assert torch.equal(topt.state[p][key], opt.state[p][key])


def test_clipped_bf16x3_step_is_bit_deterministic():
    """The bf16x3 step is bit-deterministic (tests/test_gpu_determinism.py) and stays so with clipping on:
    the norm is a fixed-order fp64 sum, not float atomics. Two runs of two clipped AdamW steps from the same
    state give the same bits in the parameters, the states, the norm and the coefficient."""
    d = dev()
    import fall_multimodal_amd as f3
    runs = []
    for _ in range(2):
        model = _model(d, "bf16x3")
        step = f3.TrainStep(model, B, optimizer=_optimizer("adamw", model, STEP_KINDS["adamw"]), max_norm=0.05)
        for k in range(2):
            step(*_batch(d, 40 + k))
        torch.cuda.synchronize()
        assert float(step.clip_coef.item()) < 1.0  # clipping was active
        runs.append([model.flat_parameters().detach().clone(), step.exp_avg.clone(), step.exp_avg_sq.clone(),
                     step.grad_norm.clone(), step.clip_coef.clone()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
