"""skip_nonfinite on the GPU (needs an MI355X): an optimizer update is applied iff every element of the
gradient it consumes is finite, decided on the device (include/fall3.h has the contract).

No new tolerance: every comparison is either a bit-equality that follows from the contract (a skipped step
stores nothing; an applied guarded step runs the unguarded flat kernel's arithmetic; a replay equals an eager
step) or goes through tests/test_gpu_optim.py's _check_step / NORM_RTOL, the fp64 yardsticks of these same
kernels. A non-finite gradient is made by poisoning one gradient element (kernel level) or one label entry
(whole step: the forward and the BN statistics stay finite, no kernel takes a data-dependent path)."""
import math

import pytest
import torch

from test_gpu_optim import B, NORM_RTOL, _batch, _check_step, _data, _keys, _model, _optimizer, dev

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
BIG = 4_194_304 + 7
KINDS = [("rmsprop", dict(lr=1e-3, alpha=0.99, eps=1e-8)),
         ("rmsprop", dict(lr=1e-3, alpha=0.99, eps=1e-8, weight_decay=0.01)),
         ("sgd", dict(lr=1e-2, momentum=0.0, weight_decay=0.01)),
         ("sgd", dict(lr=1e-2, momentum=0.9, weight_decay=0.01)),
         ("adam", dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)),
         ("adamw", dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01))]
_ids = lambda v: v if isinstance(v, (str, int)) else "-".join(f"{k}{x}" for k, x in v.items())  # noqa: E731


def bits(t):
    return t.view(torch.int32)


def _cfg(kind, hp, guard, max_norm=0.0, grad_scale=1.0):
    from fall_multimodal_amd import ops, optim as fo
    return ops.optim_config(max_norm=max_norm, grad_scale=grad_scale, skip_nonfinite=guard, **fo.hyper(kind, hp))


def _step(kind, hp, p, st, g, scalars, guard, max_norm=0.0):
    """f3_optim_step in place on torch tensors; st: the state dict in state_keys order."""
    from fall_multimodal_amd import _lib
    s = list(st.values()) + [None, None]
    _lib.check(_lib.lib().f3_optim_step(_cfg(kind, hp, guard, max_norm), _lib.ptr(p), _lib.ptr(s[0]), _lib.ptr(s[1]),
                                        _lib.ptr(g), p.numel(), _lib.ptr(scalars), _lib.stream_handle()),
               f"{kind} step")


def _words(scalars):
    """(t, clip_coef, grad_norm, skipped, last_skipped) of a block, on the host."""
    from fall_multimodal_amd import ops
    t, _, _, coef, norm = ops.scalar_views(scalars)
    skipped, last = ops.guard_views(scalars)
    return int(t.item()), float(coef.item()), float(norm.item()), int(skipped.item()), int(last.item())


def _poisons(n):
    """[(index, value), ...] lists: one bad value at 0, at n - 1 (inside the n % 4 tail that workgroup 0's
    thread 0 sums, when there is one) and, where every norm workgroup has a slice, at the first and the
    last float4 of the last workgroup's slice; and +inf with -inf together."""
    idx = {0, n - 1}
    n4 = n // 4
    chunk4 = -(-n4 // 256)
    if n4 > 255 * chunk4:
        idx |= {4 * 255 * chunk4, 4 * (n4 - 1) + 3}
    out = [[(i, v)] for i in sorted(idx) for v in (INF, -INF, NAN)]
    out.append([(0, INF), (n - 1, -INF)] if n > 1 else [(0, INF)])
    return out


# 1 / 3: a tail only; 5: one float4 and a tail; 1023: one workgroup; BIG: all 256 norm workgroups, more
# than one pass of the capped update grid, and a tail
@pytest.mark.parametrize("n", [1, 3, 5, 1023, BIG], ids=_ids)
@pytest.mark.parametrize("kind,hp", KINDS, ids=_ids)
def test_poisoned_step_is_skipped_and_the_next_one_applied(kind, hp, n):
    """1. clean, poisoned, clean. The poisoned step leaves parameters and states bit-unchanged, keeps t at 1,
    counts itself; the clean step after it is step number 2 of the fp64 formulas. The first clean step is
    run once and every poison starts from a copy of its result."""
    d = dev()
    from fall_multimodal_amd import ops
    p1, (g1, g2, g3) = _data(n, 300 + n % 89, d)
    st1 = {k: torch.zeros(n, device=d) for k in _keys(kind, hp)}
    sc1 = ops.optim_scalars(d)
    _step(kind, hp, p1, st1, g1, sc1, True)
    torch.cuda.synchronize()
    assert _words(sc1)[0] == 1 and _words(sc1)[3:] == (0, 0)
    final = None
    for poison in _poisons(n):
        p, st, sc = p1.clone(), {k: v.clone() for k, v in st1.items()}, sc1.clone()
        bad = g2.clone()
        for i, v in poison:
            bad[i] = v
        _step(kind, hp, p, st, bad, sc, True)
        torch.cuda.synchronize()
        assert torch.equal(bits(p), bits(p1)), poison
        for k in st:
            assert torch.equal(bits(st[k]), bits(st1[k])), (poison, k)
        t, coef, norm, skipped, last = _words(sc)
        assert (t, skipped, last) == (1, 1, 1) and coef == 0.0 and not math.isfinite(norm), (poison, _words(sc))
        _step(kind, hp, p, st, g3, sc, True)
        torch.cuda.synchronize()
        t, coef, norm, skipped, last = _words(sc)
        assert (t, skipped, last) == (2, 1, 0) and coef == 1.0, (poison, _words(sc))
        if final is None:
            _check_step(kind, hp, p1, st1, g3, 2, p, st, what=f"n={n} after a skip")
            ref = float(torch.linalg.vector_norm(g3.double()))
            assert abs(norm - ref) <= NORM_RTOL * ref  # grad_norm is written without clipping too
            final = (p, st, sc)
        else:  # the same inputs give the same bits, whatever was skipped in between
            assert torch.equal(bits(p), bits(final[0])) and torch.equal(bits(sc), bits(final[2]))
            for k in st:
                assert torch.equal(bits(st[k]), bits(final[1][k]))


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("n", [5, 1023, BIG], ids=_ids)
@pytest.mark.parametrize("kind,hp", KINDS, ids=_ids)
def test_finite_gradient_guard_on_equals_guard_off_bitwise(kind, hp, n, clip):
    """2. Three steps on finite gradients: the guarded step against the same configuration unguarded, bit for
    bit in parameters, states, t and clip_coef. Plain RMSprop without clipping is compared with the unguarded
    step at max_norm 1e30 (clip_coef == 1.0): the guarded route is optim_kernel, as with max_norm set."""
    d = dev()
    from fall_multimodal_amd import ops
    p0, grads = _data(n, 400 + n % 83, d)
    max_norm = 0.5 * float(torch.linalg.vector_norm(grads[0].double())) if clip else 0.0
    plain = kind == "rmsprop" and not hp.get("weight_decay", 0)
    runs = []
    for guard in (True, False):
        p, st, sc = p0.clone(), {k: torch.zeros(n, device=d) for k in _keys(kind, hp)}, ops.optim_scalars(d)
        coefs = []
        for g in grads:
            _step(kind, hp, p, st, g, sc, guard, max_norm if (guard or clip or not plain) else 1e30)
            coefs.append(ops.scalar_views(sc)[3].clone())
        torch.cuda.synchronize()
        runs.append((p, st, sc, coefs))
    (pg, sg, scg, cg), (pu, su, scu, cu) = runs
    assert torch.equal(bits(pg), bits(pu)) and not torch.equal(bits(pg), bits(p0))
    for k in sg:
        assert torch.equal(bits(sg[k]), bits(su[k])), k
    for a, b in zip(cg, cu):
        assert torch.equal(bits(a), bits(b))
    if clip:
        assert float(cg[0].item()) < 1.0
        assert torch.equal(bits(ops.scalar_views(scg)[4]), bits(ops.scalar_views(scu)[4]))  # grad_norm
    else:
        assert all(float(c.item()) == 1.0 for c in cg)
    assert _words(scg)[0] == _words(scu)[0] == 3
    assert _words(scg)[3:] == (0, 0) and _words(scu)[3:] == (0, 0)


def test_huge_finite_gradient_is_applied():
    """3. Two elements of 3e38: the norm (4.2e38) exceeds FLT_MAX, every element is finite. The decision is
    taken on the fp64 sum of squares, so the step is applied."""
    d = dev()
    from fall_multimodal_amd import ops
    hp = dict(lr=1e-3, momentum=0.0)
    n = 8
    g = torch.zeros(n, device=d)
    g[1] = 3e38
    g[6] = 3e38
    p0 = torch.linspace(-1.0, 1.0, n, device=d)
    p, sc = p0.clone(), ops.optim_scalars(d)
    _step("sgd", hp, p, {}, g, sc, True)
    torch.cuda.synchronize()
    t, coef, norm, skipped, last = _words(sc)
    print(f"huge: t={t} coef={coef} grad_norm={norm} skipped={skipped} last={last}")
    assert (t, skipped, last) == (1, 0, 0) and coef == 1.0
    assert norm == INF  # (float) of a finite fp64 norm above FLT_MAX
    _check_step("sgd", hp, p0, {}, g, 1, p, {}, what="huge finite")
    assert bool(torch.isfinite(p).all()) and float(p[1].item()) < -1e35


@pytest.mark.parametrize("kind,hp", [KINDS[4], KINDS[0]], ids=_ids)
def test_recorded_form_equals_by_value_form_bitwise(kind, hp):
    """4. f3_optim_step_hyper (what a captured step records), outside a graph: clean, poisoned, clean at
    n = 1023 against f3_optim_step on a twin set of buffers; parameters, states and the whole scalar block
    bit-equal after every step, the poisoned one skipped in both."""
    d = dev()
    from fall_multimodal_amd import _lib, ops
    n = 1023
    p0, (g1, g2, g3) = _data(n, 77, d)
    bad = g2.clone()
    bad[n - 1] = NAN
    block = ops.optim_hyper(d)
    _lib.check(_lib.lib().f3_optim_hyper_set(_cfg(kind, hp, False), _lib.ptr(block), _lib.stream_handle()), "hyper set")
    pa, pb = p0.clone(), p0.clone()
    sa = {k: torch.zeros(n, device=d) for k in _keys(kind, hp)}
    sb = {k: v.clone() for k, v in sa.items()}
    sca, scb = ops.optim_scalars(d), ops.optim_scalars(d)
    # the recorded form takes only the structure from its configuration: give it other values
    decoy = _cfg(kind, dict(hp, lr=0.7), True, grad_scale=0.321)
    for k, g in enumerate((g1, bad, g3)):
        before = pa.clone()
        s = list(sa.values()) + [None, None]
        _lib.check(_lib.lib().f3_optim_step_hyper(decoy, _lib.ptr(pa), _lib.ptr(s[0]), _lib.ptr(s[1]), _lib.ptr(g), n,
                                                  _lib.ptr(block), _lib.ptr(sca), _lib.stream_handle()), "from block")
        _step(kind, hp, pb, sb, g, scb, True)
        torch.cuda.synchronize()
        assert torch.equal(bits(pa), bits(pb)) and torch.equal(bits(sca), bits(scb)), k
        for key in sa:
            assert torch.equal(bits(sa[key]), bits(sb[key])), (k, key)
        assert torch.equal(bits(pa), bits(before)) == (k == 1)
        assert _words(sca)[0] == (1, 1, 2)[k] and _words(sca)[3:] == ((0, 0), (1, 1), (1, 0))[k]


# -- the whole step ------------------------------------------------------------------------------
STEP_HP = {"adam": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01),
           "rmsprop": dict(lr=1e-3, alpha=0.99, eps=1e-8),
           "sgd": dict(lr=1e-3, momentum=0.9, weight_decay=0.01)}
_BATCHES = {}


def _three(d):
    """b0 clean, b1 with label[0, 0] = NaN, b2 clean: made once, shared, never modified."""
    if "b" not in _BATCHES:
        bs = [_batch(d, 50 + k) for k in range(3)]
        lb = bs[1][2].clone()
        lb[0, 0] = NAN
        bs[1] = (bs[1][0], bs[1][1], lb)
        _BATCHES["b"] = bs
    return _BATCHES["b"]


def _states(step, keys):
    return {k: getattr(step, k).clone() for k in keys}


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
@pytest.mark.parametrize("mode", ["fused", "phased"])
def test_whole_step_skips_the_poisoned_batch(mode, kind):
    """5. Three TrainStep calls (bf16x3, B=32, V=18): the second batch's label holds a NaN, so its gradient
    does; its update is skipped, and the third is step number 2 of the fp64 formulas on the state the first
    left. fused: f3_net_backward_optim (one flat update after the join); phased: f3_optim_step."""
    d = dev()
    import fall_multimodal_amd as f3
    hp = STEP_HP[kind]
    model = _model(d, "bf16x3")
    step = f3.TrainStep(model, B, optimizer=_optimizer(kind, model, hp), phased=(mode == "phased"),
                        skip_nonfinite=True)
    assert step.skip_nonfinite is True and not step._legacy(step._group()) and step.fused_optimizer
    with pytest.raises(AttributeError):
        step.skip_nonfinite = False
    keys = _keys(kind, hp)
    b0, b1, b2 = _three(d)
    flat = model.flat_parameters()
    step(*b0)
    torch.cuda.synchronize()
    p1, st1 = flat.detach().clone(), _states(step, keys)
    assert int(step.step_count.item()) == 1 and int(step.last_skipped.item()) == 0 and step.skipped_steps() == 0
    step(*b1)
    torch.cuda.synchronize()
    assert torch.equal(bits(flat.detach()), bits(p1))
    for k in keys:
        assert torch.equal(bits(getattr(step, k)), bits(st1[k])), k
    assert int(step.step_count.item()) == 1 and step.skipped_steps() == 1 and int(step.last_skipped.item()) == 1
    assert not bool(torch.isfinite(step.grads).all())
    assert float(step.clip_coef.item()) == 0.0 and not math.isfinite(float(step.grad_norm.item()))
    step(*b2)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(step.grads).all())
    _check_step(kind, hp, p1, st1, step.grads, 2, flat.detach(), {k: getattr(step, k) for k in keys},
                what=f"bf16x3 {mode} after a skip")
    assert bool(torch.isfinite(flat.detach()).all())
    assert step.steps_taken() == 2 and step.skipped_steps() == 1 and int(step.last_skipped.item()) == 0


def test_captured_step_skips_on_replay():
    """6. One capture, three replays (adam, bf16x3) against an eager guarded twin fed the same batches:
    parameters, states, step_count and skipped bit-equal, and the replay of the poisoned batch leaves the
    parameters bit-unchanged. No host is in the loop of a replay: the decision is the device's."""
    d = dev()
    import fall_multimodal_amd as f3
    hp = STEP_HP["adam"]
    b0, b1, b2 = _three(d)
    model, twin = _model(d, "bf16x3", seed=61), _model(d, "bf16x3", seed=61)
    step = f3.TrainStep(model, B, optimizer=_optimizer("adam", model, hp), skip_nonfinite=True)
    tstep = f3.TrainStep(twin, B, optimizer=_optimizer("adam", twin, hp), skip_nonfinite=True)
    static = tuple(t.clone() for t in b0)
    step.capture(static[0], static[1], step.prepare(*static))
    torch.cuda.synchronize()
    assert int(step.step_count.item()) == 0 and step.skipped_steps() == 0
    flat = model.flat_parameters()
    for k, b in enumerate((b0, b1, b2)):
        before = flat.detach().clone()
        step(*b)
        tstep(*b)
        torch.cuda.synchronize()
        assert torch.equal(bits(flat.detach()), bits(before)) == (k == 1), k
        assert torch.equal(bits(flat.detach()), bits(twin.flat_parameters().detach())), k
        assert torch.equal(bits(step.exp_avg), bits(tstep.exp_avg)), k
        assert torch.equal(bits(step.exp_avg_sq), bits(tstep.exp_avg_sq)), k
        assert torch.equal(step.step_count, tstep.step_count) and torch.equal(step.skipped, tstep.skipped), k
        assert int(step.last_skipped.item()) == int(k == 1)
    assert step.steps_taken() == tstep.steps_taken() == 2 and step.skipped_steps() == tstep.skipped_steps() == 1
    assert bool(torch.isfinite(flat.detach()).all())


def test_accumulating_step_discards_a_poisoned_accumulation():
    """7. accum_iter = 2 with explicit update flags, SGD with momentum. The first pair updates; the second
    pair holds the poisoned micro-batch, so its update is skipped, yet pending returns to 0 and the reset word
    is set: the third pair's first micro-batch overwrites accum, and its update is the fp64 formula on that
    pair's gradients alone, from the momentum buffer the first update left."""
    d = dev()
    import fall_multimodal_amd as f3
    hp = STEP_HP["sgd"]
    b0, b1, b2 = _three(d)
    model = _model(d, "bf16x3")
    step = f3.TrainStep(model, B, optimizer=_optimizer("sgd", model, hp), accum_iter=2, skip_nonfinite=True)
    flat = model.flat_parameters()
    step(*b0, update=False)
    step(*b2, update=True)
    torch.cuda.synchronize()
    assert step.steps_taken() == 1 and step.skipped_steps() == 0 and step.pending == 0
    p1, buf1 = flat.detach().clone(), step.momentum_buffer.clone()
    step(*b1, update=False)  # the poisoned micro-batch
    assert step.pending == 1
    step(*b0, update=True)
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(step.accum).all())
    assert torch.equal(bits(flat.detach()), bits(p1)) and torch.equal(bits(step.momentum_buffer), bits(buf1))
    assert step.steps_taken() == 1 and step.skipped_steps() == 1 and int(step.last_skipped.item()) == 1
    assert step.pending == 0 and int(step._accum_reset.item()) == 1
    step(*b2, update=False)
    torch.cuda.synchronize()
    assert torch.equal(bits(step.accum), bits(step.grads))  # overwritten, not added to the bad sum
    step(*b0, update=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(step.accum).all())
    _check_step("sgd", hp, p1, {"momentum_buffer": buf1}, step.accum, 2, flat.detach(),
                {"momentum_buffer": step.momentum_buffer}, what="accum after a skip")
    assert step.steps_taken() == 2 and step.skipped_steps() == 1 and step.pending == 0
    assert int(step.last_skipped.item()) == 0


def test_default_is_off():
    """8. Without the keyword the step is what it was: plain RMSprop takes the legacy launches, the per-layer
    fused update is on, and an Adam step leaves the guard words (and, without max_norm, grad_norm) at 0."""
    d = dev()
    import fall_multimodal_amd as f3
    b0 = _three(d)[0]
    model = _model(d, "bf16x3")
    step = f3.TrainStep(model, B)
    assert step.skip_nonfinite is False and step._legacy(step._group()) and step.fused_optimizer
    step(*b0)
    torch.cuda.synchronize()
    assert step.steps_taken() == 1 and int(step.step_count.item()) == 0  # the legacy launches keep no device count
    assert not bool(bits(step.scalars).any())
    model = _model(d, "bf16x3")
    step = f3.TrainStep(model, B, optimizer=_optimizer("adam", model, STEP_HP["adam"]))
    assert step.skip_nonfinite is False and step.fused_optimizer
    step(*b0)
    torch.cuda.synchronize()
    assert int(step.step_count.item()) == 1 and step.skipped_steps() == 0 and int(step.last_skipped.item()) == 0
    assert float(step.grad_norm.item()) == 0.0 and float(step.clip_coef.item()) == 1.0
