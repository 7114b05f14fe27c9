"""TrainStep(ema_decay=...) on the GPU (needs an MI355X): the parameter EMA of
torch.optim.swa_utils.AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay)), kept on the device
(include/fall3.h has the contract of f3_ema_update).

The yardstick is numpy fp64: np.float32(e64 + (1.0 - decay) * (p64 - e64)) from the previous device `ema`.
The kernel performs the same three IEEE fp64 operations in the same order without contraction and rounds
once, so every comparison with it is a bit equality, with no tolerance. The one comparison with a margin is
against torch's fp64 lerp (what get_ema_multi_avg_fn runs), which is free to contract: 1 fp32 ulp. Whole
steps are compared bit for bit with the recurrence applied to their own parameter snapshots and with twin
steps (the bf16x3 step is bit-deterministic: tests/test_gpu_determinism.py)."""
import numpy as np
import pytest
import torch

from test_gpu_optim import B, _batch, _data, _model, _optimizer, dev

pytestmark = pytest.mark.gpu

# 1 / 3: a tail only; 5: one float4 and a tail; 1023: one workgroup; BIG: more than one pass of the capped
# grid (4096 workgroups of 256 float4s) and a tail
BIG = 4_194_311
SIZES = [1, 3, 5, 1023, BIG]
GUARD = 32  # floats either side of `ema` inside its allocation (a multiple of 4: ema stays 16-byte aligned)


def bits(t):
    return t.view(torch.int32)


def np_lerp(e32, p32, decay):
    """The contract's expression in numpy fp64, rounded to fp32 once."""
    e64, p64 = e32.astype(np.float64), p32.astype(np.float64)
    return np.float32(e64 + (1.0 - decay) * (p64 - e64))


def same_bits(a32, b32):
    return np.array_equal(np.asarray(a32, dtype=np.float32).view(np.int32), np.asarray(b32, dtype=np.float32).view(np.int32))


def host(t):
    return t.detach().cpu().numpy().copy()


def _block(d, decay):
    from fall_multimodal_amd import _lib, ops
    st = ops.ema_state(d)
    _lib.check(_lib.lib().f3_ema_set_decay(_lib.ptr(st), decay, _lib.stream_handle()), "ema decay")
    return st


def _update(ema, params, st, n=None):
    from fall_multimodal_amd import _lib
    _lib.check(_lib.lib().f3_ema_update(_lib.ptr(ema), _lib.ptr(params), ema.numel() if n is None else n, _lib.ptr(st),
                                        _lib.stream_handle()), "ema update")


def _guarded(n, d, seed):
    """(whole allocation, the n-float `ema` view inside it): random bits everywhere, `ema`'s included (the
    first update must overwrite them)."""
    gen = torch.Generator().manual_seed(seed)
    whole = torch.randn(n + 2 * GUARD, generator=gen).to(d)
    return whole, whole[GUARD:GUARD + n]


def _sequence(n, decay, d, updates=4):
    """`updates` f3_ema_update calls with fresh params; the device ema after each, on the host."""
    from fall_multimodal_amd import ops
    whole, ema = _guarded(n, d, 11 + n % 97)
    before = host(whole)
    _, params = _data(n, 500 + n % 89, d, steps=updates)
    kept = [host(p) for p in params]
    st = _block(d, decay)
    out = []
    for p in params:
        _update(ema, p, st)
        out.append(host(ema))
    torch.cuda.synchronize()
    count, dec = ops.ema_views(st)
    return out, kept, [host(p) for p in params], before, host(whole), int(count.item()), float(dec.item())


# ---- the kernel --------------------------------------------------------------------------------
@pytest.mark.parametrize("decay", [0.9, 0.999])
@pytest.mark.parametrize("n", SIZES)
def test_update_matches_numpy_fp64_bitwise(n, decay):
    """1. Four updates with fresh params: the first copies params' bits, each later one has the bits of the
    numpy expression from the previous device ema; n_averaged == 4; params and the guard elements either
    side of ema keep their bits."""
    d = dev()
    emas, p_before, p_after, whole0, whole1, count, dec = _sequence(n, decay, d)
    assert same_bits(emas[0], p_before[0])
    for k in range(1, 4):
        want = np_lerp(emas[k - 1], p_before[k], decay)
        diff = int((want.view(np.int32) != emas[k].view(np.int32)).sum())
        print(f"n={n} decay={decay} update {k + 1}: {diff} of {n} elements differ in bits")
        assert diff == 0
    assert count == 4 and dec == decay
    for a, b in zip(p_before, p_after):
        assert same_bits(a, b)
    assert same_bits(whole0[:GUARD], whole1[:GUARD]) and same_bits(whole0[GUARD + n:], whole1[GUARD + n:])


@pytest.mark.parametrize("n", [5, 1023])
def test_decay_one_and_decay_zero(n):
    """2. decay 1.0 leaves ema's bits alone from the second update on; decay 0.0 is the same numpy expression
    (e + 1.0 (p - e), which need not round to p), not a copy of params."""
    d = dev()
    emas, p_before, _, _, _, count, _ = _sequence(n, 1.0, d)
    assert same_bits(emas[0], p_before[0])
    for k in range(1, 4):
        assert same_bits(emas[k], emas[0])
    assert count == 4
    emas, p_before, _, _, _, count, _ = _sequence(n, 0.0, d)
    assert same_bits(emas[0], p_before[0])
    for k in range(1, 4):
        assert same_bits(emas[k], np_lerp(emas[k - 1], p_before[k], 0.0))
    assert count == 4


def test_set_decay_takes_effect_and_a_refused_value_leaves_the_block():
    """3. f3_ema_set_decay between two updates is read by the second; a refused value (F3_EINVAL, nothing
    launched) leaves the block's 16 bytes as they were."""
    d = dev()
    from fall_multimodal_amd import _lib
    n = 1023
    _, ema = _guarded(n, d, 5)
    _, (p0, p1, p2) = _data(n, 41, d)
    st = _block(d, 0.999)
    _update(ema, p0, st)
    _update(ema, p1, st)
    e1 = host(ema)
    assert same_bits(e1, np_lerp(host(p0), host(p1), 0.999))
    before = st.clone()
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        assert _lib.lib().f3_ema_set_decay(_lib.ptr(st), bad, _lib.stream_handle()) == _lib.F3_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(st, before) and int(st[0].item()) == 2
    _lib.check(_lib.lib().f3_ema_set_decay(_lib.ptr(st), 0.5, _lib.stream_handle()), "ema decay")
    _update(ema, p2, st)
    torch.cuda.synchronize()
    assert same_bits(host(ema), np_lerp(e1, host(p2), 0.5))
    assert not same_bits(host(ema), np_lerp(e1, host(p2), 0.999))
    assert int(st[0].item()) == 3 and float(st[1:2].view(torch.float64).item()) == 0.5


def _ordered(a32):
    """fp32 bits as integers in the order of the values: neighbours differ by 1."""
    i = a32.view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


@pytest.mark.parametrize("decay", [0.9, 0.999])
@pytest.mark.parametrize("n", SIZES)
def test_update_within_one_ulp_of_torch_fp64_lerp(n, decay):
    """4. One update (after the copying one) against torch.lerp(ema.double(), params.double(), 1 - decay)
    .float() on the CPU, what get_ema_multi_avg_fn runs: within 1 fp32 ulp everywhere (torch's lerp is free
    to contract; the numpy yardstick itself stays inside the same bound)."""
    d = dev()
    _, ema = _guarded(n, d, 23)
    _, (p0, p1) = _data(n, 700 + n % 83, d, steps=2)
    st = _block(d, decay)
    _update(ema, p0, st)
    _update(ema, p1, st)
    torch.cuda.synchronize()
    want = torch.lerp(p0.cpu().double(), p1.cpu().double(), 1 - decay).float().numpy()
    got = host(ema)
    worst = int(np.abs(_ordered(got) - _ordered(want)).max())
    yard = int(np.abs(_ordered(np_lerp(host(p0), host(p1), decay)) - _ordered(want)).max())
    print(f"n={n} decay={decay}: kernel vs torch fp64 lerp {worst} ulp, numpy yardstick vs torch {yard} ulp")
    assert worst <= 1


@pytest.mark.parametrize("n", [1023, BIG])
def test_same_sequence_twice_gives_identical_bits(n):
    """5. No atomics, a fixed evaluation order: two runs of the same sequence agree bit for bit."""
    d = dev()
    a = _sequence(n, 0.999, d)
    b = _sequence(n, 0.999, d)
    for x, y in zip(a[0], b[0]):
        assert same_bits(x, y)
    assert a[5] == b[5] == 4


def test_zero_elements_only_advances_the_count():
    d = dev()
    _, ema = _guarded(8, d, 3)
    keep = host(ema)
    p = torch.ones(8, device=d)
    st = _block(d, 0.9)
    _update(ema, p, st, n=0)
    _update(ema, p, st, n=0)
    torch.cuda.synchronize()
    assert int(st[0].item()) == 2 and same_bits(host(ema), keep)


# ---- the whole step ------------------------------------------------------------------------------
DECAY = 0.999
ROUTES = {  # the three routes of an eager step
    "rmsprop-fused-per-layer": ("rmsprop", None, {}),
    "adamw-clipped-flat": ("adamw", dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01), dict(max_norm=1.0)),
    "sgd-phased": ("sgd", dict(lr=1e-3, momentum=0.9, weight_decay=0.01), dict(phased=True)),
}
_BATCHES = {}


def _batches(d):
    """Four clean batches and one whose label holds a NaN: made once, shared, never modified."""
    if "b" not in _BATCHES:
        bs = [_batch(d, 80 + k) for k in range(4)]
        lb = bs[1][2].clone()
        lb[0, 0] = float("nan")
        _BATCHES["b"] = (bs, (bs[1][0], bs[1][1], lb))
    return _BATCHES["b"]


def _make(d, kind="rmsprop", hp=None, seed=9, **kw):
    import fall_multimodal_amd as f3
    model = _model(d, "bf16x3", seed=seed)
    opt = _optimizer(kind, model, hp) if hp is not None else None
    return model, f3.TrainStep(model, B, optimizer=opt, **kw)


@pytest.mark.parametrize("route", list(ROUTES))
def test_eager_step_follows_the_recurrence_and_never_writes_the_model(route):
    """6. After every step `ema` equals the numpy recurrence applied to the parameter snapshots, bit for bit,
    n_averaged the step count; the parameters are those of a twin step built without ema_decay."""
    d = dev()
    kind, hp, kw = ROUTES[route]
    model, step = _make(d, kind, hp, ema_decay=DECAY, **kw)
    twin, tstep = _make(d, kind, hp, **kw)
    if route == "rmsprop-fused-per-layer":
        assert step.fused_optimizer and step._legacy(step._group())
    assert step.ema_decay == DECAY and tstep.ema is None and tstep.ema_state is None and tstep.ema_decay is None
    flat = model.flat_parameters()
    assert step.ema.data_ptr() != flat.data_ptr() and torch.equal(bits(step.ema), bits(flat.detach()))
    assert int(step.n_averaged.item()) == 0 and step.n_averaged.dtype == torch.int64
    bs, _ = _batches(d)
    want = None
    for k, b in enumerate(bs[:3]):
        step(*b)
        tstep(*b)
        torch.cuda.synchronize()
        p = host(flat)
        want = p if k == 0 else np_lerp(want, p, DECAY)
        assert same_bits(host(step.ema), want), (route, k)
        assert int(step.n_averaged.item()) == k + 1
        assert torch.equal(bits(flat.detach()), bits(twin.flat_parameters().detach())), (route, k)
    assert not same_bits(want, host(flat))  # the average lags the parameters
    with pytest.raises(ValueError):
        tstep.ema_decay = 0.9
    with pytest.raises(ValueError):
        tstep.ema_update()
    with pytest.raises(ValueError):
        step.ema_decay = 1.5


def test_captured_step_advances_the_average_on_replay_and_follows_a_new_decay():
    """7. One capture, then replays against an eager twin on the same batches: ema and parameters bit-equal,
    n_averaged advancing per replay (capture() itself leaves the average alone); step.ema_decay = 0.9 after
    capture is followed by the next replay without recapturing."""
    d = dev()
    hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    model, step = _make(d, "adam", hp, seed=61, ema_decay=DECAY)
    twin, tstep = _make(d, "adam", hp, seed=61, ema_decay=DECAY)
    bs, _ = _batches(d)
    static = tuple(t.clone() for t in bs[0])
    start = model.flat_parameters().detach().clone()
    step.capture(static[0], static[1], step.prepare(*static))
    torch.cuda.synchronize()
    assert int(step.n_averaged.item()) == 0 and torch.equal(bits(step.ema), bits(start))
    flat = model.flat_parameters()
    for k, b in enumerate(bs[:3]):
        step(*b)
        tstep(*b)
        torch.cuda.synchronize()
        assert torch.equal(bits(flat.detach()), bits(twin.flat_parameters().detach())), k
        assert torch.equal(bits(step.ema), bits(tstep.ema)), k
        assert int(step.n_averaged.item()) == int(tstep.n_averaged.item()) == k + 1
    e3 = host(step.ema)
    graph = step.graph
    step.ema_decay = 0.9
    tstep.ema_decay = 0.9
    step(*bs[3])
    tstep(*bs[3])
    torch.cuda.synchronize()
    assert step.graph is graph and step.ema_decay == 0.9
    assert torch.equal(bits(step.ema), bits(tstep.ema)) and int(step.n_averaged.item()) == 4
    assert same_bits(host(step.ema), np_lerp(e3, host(flat), 0.9))
    assert not same_bits(host(step.ema), np_lerp(e3, host(flat), DECAY))


def test_accumulating_step_counts_update_calls_only():
    """8. accum_iter = 2 with explicit update flags: the average moves on update calls only."""
    d = dev()
    model, step = _make(d, ema_decay=DECAY, accum_iter=2)
    bs, _ = _batches(d)
    flat = model.flat_parameters()
    want, count = host(step.ema), 0
    for k, (b, upd) in enumerate(zip([bs[0], bs[1], bs[2], bs[3], bs[0]], [False, True, False, False, True])):
        step(*b, update=upd)
        torch.cuda.synchronize()
        if upd:
            want = host(flat) if count == 0 else np_lerp(want, host(flat), DECAY)
            count += 1
        assert int(step.n_averaged.item()) == count, k
        assert same_bits(host(step.ema), want), k
    assert count == 2 and step.steps_taken() == 2


def test_a_skipped_update_still_moves_the_average():
    """9. skip_nonfinite=True with one poisoned label entry: the parameters keep their bits and last_skipped
    is 1, yet n_averaged advances and ema is the lerp toward the unchanged parameters, as torch's loop calls
    ema.update_parameters(model) whether or not scaler.step applied."""
    d = dev()
    hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    model, step = _make(d, "adam", hp, ema_decay=0.9, skip_nonfinite=True)
    bs, bad = _batches(d)
    flat = model.flat_parameters()
    step(*bs[0])
    step(*bs[2])
    torch.cuda.synchronize()
    p2, e2 = host(flat), host(step.ema)
    assert int(step.n_averaged.item()) == 2 and not same_bits(p2, e2)
    step(*bad)
    torch.cuda.synchronize()
    assert same_bits(host(flat), p2) and int(step.last_skipped.item()) == 1 and step.skipped_steps() == 1
    assert int(step.n_averaged.item()) == 3 and step.steps_taken() == 2
    assert same_bits(host(step.ema), np_lerp(e2, p2, 0.9))
    assert not same_bits(host(step.ema), e2)
    assert bool(torch.isfinite(step.ema).all())


def test_swap_ema_exchanges_in_place_and_evaluates_the_average(tmp_path):
    """10. Inside swap_ema() the model holds the former ema bits at the same address and the step refuses to
    run; after exit, also after an exception in the body, both buffers are bit-restored. valid_device
    inside the context returns what a fresh model loaded from ema_state_dict() returns, also through
    evaluate.save_best's file format."""
    d = dev()
    from fall_multimodal_amd import evaluate
    model, step = _make(d, ema_decay=0.9)
    bs, _ = _batches(d)
    for b in bs[:3]:
        step(*b)
    torch.cuda.synchronize()
    flat = model.flat_parameters()
    p0, e0 = flat.detach().clone(), step.ema.clone()
    ptr_p, ptr_e = flat.data_ptr(), step.ema.data_ptr()
    assert not torch.equal(bits(p0), bits(e0))
    sd = step.ema_state_dict()
    ref = model.state_dict()
    assert list(sd.keys()) == list(ref.keys())
    names = {n for n, _ in model.named_parameters()}
    for k, v in ref.items():
        assert sd[k].shape == v.shape and sd[k].dtype == v.dtype, k
        if k not in names:
            assert torch.equal(sd[k], v), k  # the buffers are the model's
    loader = [bs[3], bs[0]]
    with step.swap_ema() as m:
        assert m is model
        assert model.flat_parameters().data_ptr() == ptr_p and step.ema.data_ptr() == ptr_e
        assert torch.equal(bits(flat.detach()), bits(e0)) and torch.equal(bits(step.ema), bits(p0))
        with pytest.raises(RuntimeError):
            step(*bs[0])
        inside = evaluate.valid_device(model, loader)
    assert torch.equal(bits(flat.detach()), bits(p0)) and torch.equal(bits(step.ema), bits(e0))
    with pytest.raises(KeyError):
        with step.swap_ema():
            raise KeyError("body")
    assert torch.equal(bits(flat.detach()), bits(p0)) and torch.equal(bits(step.ema), bits(e0))
    assert int(step.n_averaged.item()) == 3
    fresh = _model(d, "bf16x3", seed=3)
    fresh.load_state_dict(sd)
    assert evaluate.valid_device(fresh, loader) == inside
    assert evaluate.valid_device(model, loader) != inside  # the raw weights give another loss
    path = str(tmp_path / "best_ema.pt")
    torch.save({"model_weight": {k: v.detach().cpu() for k, v in sd.items()}}, path)
    again = evaluate.load_best(_model(d, "bf16x3", seed=4), path)
    assert evaluate.valid_device(again, loader) == inside
    step(*bs[0])  # the step runs again after the context
    torch.cuda.synchronize()
    assert int(step.n_averaged.item()) == 4


def test_checkpoint_round_trip_continues_with_the_same_bits():
    """11. ema_checkpoint() -> a new TrainStep -> load_ema_checkpoint(): buffer, count and decay are
    restored, and the next update gives the bits of the uninterrupted run."""
    d = dev()
    model, step = _make(d, ema_decay=DECAY)
    bs, _ = _batches(d)
    step(*bs[0])
    step(*bs[1])
    ck = step.ema_checkpoint()
    assert ck["n_averaged"] == 2 and ck["decay"] == DECAY
    assert list(ck["params"]) == [n for n, _ in model.named_parameters()]
    assert all(not t.is_cuda for t in ck["params"].values())
    model2, step2 = _make(d, ema_decay=0.5)
    step2.load_ema_checkpoint(ck)
    torch.cuda.synchronize()
    assert step2.ema_decay == DECAY and int(step2.n_averaged.item()) == 2
    # the checkpoint holds the parameters: the < 4 floats of alignment padding after each are not compared
    held = torch.zeros(step.ema.numel(), dtype=torch.bool, device=d)
    for _, shape, off in model.param_views():
        held[off:off + int(np.prod(shape))] = True
    assert torch.equal(bits(step2.ema)[held], bits(step.ema)[held])
    step(*bs[2])  # the uninterrupted run
    with torch.no_grad():
        model2.flat_parameters().copy_(model.flat_parameters())
    step2.ema_update()
    torch.cuda.synchronize()
    assert torch.equal(bits(step2.ema)[held], bits(step.ema)[held])
    assert int(step2.n_averaged.item()) == int(step.n_averaged.item()) == 3
    bad = dict(ck, decay=1.5)
    with pytest.raises(ValueError):
        step2.load_ema_checkpoint(bad)
    assert step2.ema_decay == DECAY and int(step2.n_averaged.item()) == 3
