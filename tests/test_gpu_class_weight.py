"""Class-weighted cross-entropy on the MI355X: f3_soft_ce_w against torch.nn.functional.cross_entropy in fp64
(both of torch's rules: probability targets divided by N, class indices divided by the sum of the live
rows' weights), its exact relations to f3_soft_ce_ex, and the weights inside TrainStep, the three side
steps and the eval loops. Cases, yardstick and gates: tests/class_weight_ref.py (shared with the CPU
emulation of tests/test_class_weight.py)."""
import numpy as np
import pytest
import torch

from oracle import model_cpu as oc
from oracle.prng import synthetic_batch
from tests import class_weight_ref as R

pytestmark = pytest.mark.gpu

EINVAL = 1001
B = 8


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda")


def bits(t):
    return t.contiguous().view(torch.int32)


def _forms(label_t, both=None):
    soft, idx = (label_t, None) if (label_t is not None and label_t.dim() == 2) else (None, label_t)
    return (soft, idx) if both is None else both


def run_w(out_t, label_t, w_t, eps, loss_t, dout_t, N=None, C=None, both=None):
    """f3_soft_ce_w's status; a 2-D label is the soft form, a 1-D one the index form."""
    from fall_multimodal_amd._lib import lib, ptr, stream_handle
    soft, idx = _forms(label_t, both)
    return lib().f3_soft_ce_w(ptr(out_t), ptr(soft), ptr(idx), ptr(w_t), out_t.shape[0] if N is None else N,
                              out_t.shape[1] if C is None else C, eps, ptr(loss_t), ptr(dout_t), stream_handle())


def run_ex(out_t, label_t, eps, loss_t, dout_t):
    from fall_multimodal_amd._lib import lib, ptr, stream_handle
    soft, idx = _forms(label_t)
    return lib().f3_soft_ce_ex(ptr(out_t), ptr(soft), ptr(idx), out_t.shape[0], out_t.shape[1], eps, ptr(loss_t),
                               ptr(dout_t), stream_handle())


def nan_pair(d, N, C):
    return torch.full((1,), float("nan"), device=d), torch.full((N, C), float("nan"), device=d)


def weighted(d, out, label, w, eps):
    """(loss tensor, dout tensor) of one f3_soft_ce_w call on host arrays."""
    out_t, label_t, w_t = (torch.from_numpy(x).to(d) for x in (out, label, w))
    loss_t, dout_t = nan_pair(d, *out.shape)
    assert run_w(out_t, label_t, w_t, eps, loss_t, dout_t) == 0
    return loss_t, dout_t


# ---- 1. the kernel against fp64 torch -------------------------------------------------------------
@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("C", R.CLASSES)
def test_soft_ce_w_matches_fp64_torch(C, form):
    """Every N of class_weight_ref.BATCHES x every eps of SMOOTHINGS. loss and dout start as NaN and come back
    finite and inside the gates; ignored rows' dout is exactly 0; dout = NULL gives the same loss bits and
    writes nothing around the loss word; the inputs keep their bits; a second run gives the same bits."""
    d = dev()
    worst_l = worst_d = 0.0
    for N in R.BATCHES:
        for eps in R.SMOOTHINGS:
            out, label, w = R.make_case(N, C, form, eps)
            out_t, label_t, w_t = (torch.from_numpy(x).to(d) for x in (out, label, w))
            loss_t, dout_t = nan_pair(d, N, C)
            assert run_w(out_t, label_t, w_t, eps, loss_t, dout_t) == 0
            loss, dout = float(loss_t.cpu()[0]), dout_t.cpu().numpy()
            assert np.isfinite(loss) and np.isfinite(dout).all(), (N, C, eps, form)
            rl, rd = R.gate_ratios(loss, dout, out, label, w, eps)
            worst_l, worst_d = max(worst_l, rl), max(worst_d, rd)
            assert rl <= 1.0, (N, C, eps, form, loss, rl)
            assert rd <= 1.0, (N, C, eps, form, rd)
            if label.ndim == 1:
                dead = ~R.live_rows(label, C)
                assert not dout.view(np.uint32)[dead].any(), (N, C, eps, form)  # +0.0 in every word
            # loss only: a sentinel-filled buffer around the loss word stays as it was
            guard = torch.full((129,), -7.5, device=d)
            assert run_w(out_t, label_t, w_t, eps, guard[64:65], None) == 0
            assert torch.equal(bits(guard[64:65]), bits(loss_t)), (N, C, eps, form)
            assert bool((torch.cat([guard[:64], guard[65:]]) == -7.5).all()), (N, C, eps, form)
            # the same bits again, and the inputs are only read
            loss2, dout2 = nan_pair(d, N, C)
            assert run_w(out_t, label_t, w_t, eps, loss2, dout2) == 0
            assert torch.equal(bits(loss2), bits(loss_t)) and torch.equal(bits(dout2), bits(dout_t))
            assert torch.equal(bits(out_t).cpu(), bits(torch.from_numpy(out)))
            assert torch.equal(w_t.cpu().view(torch.int32), torch.from_numpy(w).view(torch.int32))
            if label.ndim == 1:
                assert torch.equal(label_t.cpu(), torch.from_numpy(label))
            else:
                assert torch.equal(bits(label_t).cpu(), bits(torch.from_numpy(label)))
    print(f"C={C} {form}: worst loss gate ratio {worst_l:.4f}, worst dout gate ratio {worst_d:.4f}")


# ---- 2. exact relations to f3_soft_ce_ex -------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 11, 16, 17])
@pytest.mark.parametrize("N", [8, 300, 5000])
def test_uniform_weights_are_exact(N, C):
    """Derived, no tolerance. f3_soft_ce_ex and f3_soft_ce_w run one row function whose roundings are written
    out (fp contraction off, explicit fmaf), with a = y' * w for y' and m for sum y'. Weights 1: a = y'
    exactly, and W = N exactly in fp64, so both rules give f3_soft_ce_ex's bits (all indices in range).
    Weights 2: a, m, every fused product and every sum double exactly, so the probability rule gives exactly
    twice the unweighted loss and dout; under the index rule W = 2N and 2x / 2N = x / N exactly: the
    unweighted bits. C = 2 and 11 are the two datasets' class counts, 16 the widest register row, 17 the
    row-in-memory path; N = 8 and 300 the single-workgroup form, 5000 the large-batch one."""
    d = dev()
    for eps in (0.0, 0.1):
        rng = np.random.default_rng([N, C, int(10 * eps)])
        out = rng.uniform(-4.0, 4.0, (N, C)).astype(np.float32)
        soft = rng.random((N, C)).astype(np.float32)
        soft /= soft.sum(1, keepdims=True)
        idx = rng.integers(0, C, N).astype(np.int64)
        out_t = torch.from_numpy(out).to(d)
        for label in (soft, idx):
            label_t = torch.from_numpy(label).to(d)
            loss0, dout0 = nan_pair(d, N, C)
            assert run_ex(out_t, label_t, eps, loss0, dout0) == 0
            assert np.isfinite(float(loss0.cpu()[0]))
            form = "soft" if label.ndim == 2 else "index"
            for wv in (1.0, 2.0):
                w_t = torch.full((C,), wv, device=d)
                loss1, dout1 = nan_pair(d, N, C)
                assert run_w(out_t, label_t, w_t, eps, loss1, dout1) == 0
                twice = wv == 2.0 and form == "soft"
                want_l, want_d = (loss0 * 2.0, dout0 * 2.0) if twice else (loss0, dout0)
                assert torch.equal(bits(loss1), bits(want_l)), (N, C, eps, form, wv, float(loss1.cpu()[0]),
                                                                float(want_l.cpu()[0]))
                assert torch.equal(bits(dout1), bits(want_d)), (N, C, eps, form, wv)


# ---- 3. a batch that makes the 1024 workgroups stride ----------------------------------------------------
def test_large_batch_strides_reproducibly_inside_the_gates():
    d = dev()
    N, C, eps = 262145, 2, 0.1
    out, label, w = R.make_case(N, C, "index_ignore", eps)
    out_t, label_t, w_t = (torch.from_numpy(x).to(d) for x in (out, label, w))
    runs = []
    for _ in range(2):
        loss_t, dout_t = nan_pair(d, N, C)
        assert run_w(out_t, label_t, w_t, eps, loss_t, dout_t) == 0
        runs.append((loss_t, dout_t))
    assert torch.equal(bits(runs[0][0]), bits(runs[1][0])) and torch.equal(bits(runs[0][1]), bits(runs[1][1]))
    loss, dout = float(runs[0][0].cpu()[0]), runs[0][1].cpu().numpy()
    assert np.isfinite(loss) and np.isfinite(dout).all()
    rl, rd = R.gate_ratios(loss, dout, out, label, w, eps)
    print(f"N={N} C={C}: loss gate ratio {rl:.4f}, dout gate ratio {rd:.4f}")
    assert rl <= 1.0 and rd <= 1.0, (rl, rd)
    assert not dout.view(np.uint32)[~R.live_rows(label, C)].any()
    only = torch.full((1,), float("nan"), device=d)
    assert run_w(out_t, label_t, w_t, eps, only, None) == 0
    assert torch.equal(bits(only), bits(runs[0][0]))


# ---- 4. W == 0 --------------------------------------------------------------------------------------
def test_no_live_row_gives_nan_as_torch():
    d = dev()
    out_t = torch.zeros(3, 11, device=d)
    idx = torch.tensor([-100, 11, -1], dtype=torch.int64, device=d)
    w_t = torch.ones(11, device=d)
    loss_t, dout_t = torch.zeros(1, device=d), torch.zeros(3, 11, device=d)
    assert run_w(out_t, idx, w_t, 0.1, loss_t, dout_t) == 0
    assert bool(torch.isnan(loss_t).all()) and bool(torch.isnan(dout_t).all())


# ---- 5. refusals ------------------------------------------------------------------------------------
def test_soft_ce_w_refuses_bad_arguments():
    d = dev()
    out_t = torch.zeros(4, 11, device=d)
    soft = torch.full((4, 11), 1.0 / 11, device=d)
    idx = torch.zeros(4, dtype=torch.int64, device=d)
    w_t = torch.ones(11, device=d)
    loss_t, dout_t = torch.full((1,), -7.5, device=d), torch.full((4, 11), -7.5, device=d)
    assert run_w(out_t, soft, None, 0.1, loss_t, dout_t) == EINVAL                      # null weights
    assert run_w(out_t, None, w_t, 0.1, loss_t, dout_t, both=(soft, idx)) == EINVAL     # both label forms
    assert run_w(out_t, None, w_t, 0.1, loss_t, dout_t, both=(None, None)) == EINVAL    # neither
    wide = torch.zeros(4, 65, device=d)
    assert run_w(wide, torch.zeros(4, 65, device=d), torch.ones(65, device=d), 0.1, loss_t,
                 torch.zeros(4, 65, device=d)) == EINVAL                                # C = 65
    for eps in (1.5, -0.1, float("nan"), float("inf")):
        assert run_w(out_t, soft, w_t, eps, loss_t, dout_t) == EINVAL, eps
    assert run_w(out_t, soft, w_t, 0.1, loss_t, dout_t, N=0) == EINVAL
    assert run_w(out_t, soft, w_t, 0.1, loss_t, dout_t, C=0) == EINVAL
    assert run_w(out_t, soft, w_t, 0.1, None, dout_t) == EINVAL
    torch.cuda.synchronize()
    assert float(loss_t.cpu()[0]) == -7.5 and bool((dout_t == -7.5).all())  # a refused call launches nothing
    assert run_w(out_t, soft, w_t, 0.1, loss_t, dout_t) == 0 and run_w(out_t, idx, w_t, 1.0, loss_t, dout_t) == 0


# ---- the model (the 3-stream spec and B = 8 of tests/test_gpu_accum_smoothing.py) ---------------------------
SPEC = oc.Spec(model="two_stgcan_bilstm", layout="coco_mmpose", num_class=11, sensor_dim=6)


def _net(d, st):
    import fall_multimodal_amd as f3
    model = f3.TwoStreamSTGCAN_BiLSTM(3, {"layout": "coco_mmpose", "strategy": "spatial"}, 11, 6, device=d,
                                      precision="bf16x3")
    model.load_state_dict(st)
    return model


@pytest.fixture(scope="module")
def state():
    return oc.init_state(SPEC, 61)


@pytest.fixture(scope="module")
def batches():
    d = dev()
    return [[torch.from_numpy(x).to(d) for x in synthetic_batch(B, 18, 11, 6, 70 + i)] for i in range(4)]


def _weights(seed, C=11):
    return R.make_weights(np.random.default_rng(seed), C)


def _same_state(model, twin):
    assert torch.equal(model.flat_parameters(), twin.flat_parameters())
    assert torch.equal(model._flat_buffers, twin._flat_buffers)


# ---- 6. TrainStep -----------------------------------------------------------------------------------
_ONES = {}


def _ones_run(eps, state, batches):
    """Three steps of TrainStep(class_weight=ones) beside a default twin, run once per eps and shared: per step
    the two loss words and whether dout and grads agree bit for bit, then whether parameters and buffers do."""
    if eps not in _ONES:
        import fall_multimodal_amd as f3
        d = dev()
        model, twin = _net(d, state), _net(d, state)
        step = f3.TrainStep(model, B, lr=1e-3, label_smoothing=eps, class_weight=np.ones(11))
        tstep = f3.TrainStep(twin, B, lr=1e-3, label_smoothing=eps)
        assert tstep.class_weight is None and step.class_weight.tolist() == [1.0] * 11
        rec = {"loss": [], "dout": [], "grads": []}
        for sk, se, lb in batches[:3]:
            step(sk, se, lb)
            tstep(sk, se, lb)
            rec["loss"].append((int(bits(step.loss).item()), int(bits(tstep.loss).item())))
            rec["dout"].append(torch.equal(bits(step.dout), bits(tstep.dout)))
            rec["grads"].append(torch.equal(bits(step.grads), bits(tstep.grads)))
        torch.cuda.synchronize()
        rec["params"] = torch.equal(model.flat_parameters(), twin.flat_parameters())
        rec["buffers"] = torch.equal(model._flat_buffers, twin._flat_buffers)
        rec["steps"] = (step.steps_taken(), tstep.steps_taken())
        _ONES[eps] = rec
    return _ONES[eps]


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_all_ones_weights_train_as_the_default_step(eps, state, batches):
    """dout, the gradient, the parameters and the BN buffers of three steps: the default twin's bits."""
    rec = _ones_run(eps, state, batches)
    assert rec["dout"] == [True] * 3 and rec["grads"] == [True] * 3, rec
    assert rec["params"] and rec["buffers"] and rec["steps"] == (3, 3), rec


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_all_ones_weights_log_the_default_steps_loss(eps, state, batches):
    """The loss word of the same three steps. At eps = 0.1 the twin's launch is f3_net_loss_ex, at eps = 0
    f3_net_loss (ce_kernel, head.hip): the loss row fuses its products exactly where ce_kernel's compiled code
    does, so all three kernels log the same word."""
    rec = _ones_run(eps, state, batches)
    print(f"eps={eps}: loss words (all-ones weights, default) per step {rec['loss']}")
    assert all(a == b for a, b in rec["loss"]), rec["loss"]


def test_step_loss_and_dout_are_the_weighted_ones(state, batches):
    """loss and dout carry f3_soft_ce_w's bits for step.out and pass the fp64 gates; metrics=True logs them; a
    default twin given the weighted dout produces the weighted step's gradient: the backward consumes it."""
    import fall_multimodal_amd as f3
    d = dev()
    w = _weights(5)
    eps = 0.1
    model, twin = _net(d, state), _net(d, state)
    step = f3.TrainStep(model, B, lr=1e-3, label_smoothing=eps, class_weight=w, metrics=True)
    tstep = f3.TrainStep(twin, B, lr=1e-3)
    np.testing.assert_array_equal(step.class_weight.cpu().numpy(), w)
    # the backward consumes the weighted dout (before any update: the twins hold the same parameters)
    sk, se, lb = batches[3]
    step.forward_loss(sk, se, step.prepare(sk, se, lb))
    step.backward_phase(0)
    tstep.forward_loss(sk, se, tstep.prepare(sk, se, lb))
    assert not torch.equal(bits(tstep.dout), bits(step.dout))
    tstep.dout.copy_(step.dout)
    tstep.backward_phase(0)
    torch.cuda.synchronize()
    assert torch.equal(bits(tstep.grads), bits(step.grads)) and bool(step.grads.any())
    step.metrics.reset()
    loss_sum = np.float64(0.0)
    for sk, se, lb in batches[:3]:
        step(sk, se, lb)
        torch.cuda.synchronize()
        out, label = step.out.cpu().numpy(), lb.cpu().numpy()
        loss_t, dout_t = weighted(d, out, label, w, eps)
        assert torch.equal(bits(step.loss), bits(loss_t)) and torch.equal(bits(step.dout), bits(dout_t))
        loss = step.loss.cpu().numpy()[0]
        rl, rd = R.gate_ratios(float(loss), step.dout.cpu().numpy(), out, label, w, eps)
        print(f"step loss {float(loss)!r}: loss gate ratio {rl:.4f}, dout gate ratio {rd:.4f}")
        assert rl <= 1.0 and rd <= 1.0, (rl, rd)
        loss_sum = loss_sum + np.float64(loss)
    blk = step.metrics.block.cpu().numpy()
    assert int(blk[1]) == 3 and int(blk[2]) == 3 * B
    assert blk[0:1].view(np.float64)[0].tobytes() == loss_sum.tobytes()  # the weighted loss is what is logged
    assert step.metrics.result()["loss"] == float(loss_sum / 3)


def test_accumulating_weighted_step_matches_a_twin_driven_by_hand(state, batches):
    """accum_iter = 2 with weights and smoothing, four batches after begin_epoch(4): updates after batches 0,
    2 and 3; the twin (same weights, same smoothing) is folded by hand as in tests/test_gpu_accum_smoothing.py."""
    import fall_multimodal_amd as f3
    from fall_multimodal_amd.train import accum_updates
    d = dev()
    w = _weights(6)
    model, twin = _net(d, state), _net(d, state)
    step = f3.TrainStep(model, B, lr=1e-3, label_smoothing=0.1, class_weight=w, accum_iter=2)
    tstep = f3.TrainStep(twin, B, lr=1e-3, label_smoothing=0.1, class_weight=w)
    due = accum_updates(4, 2)
    assert due == [True, False, True, True]
    step.begin_epoch(4)
    exp, fresh = None, True
    for i, (sk, se, lb) in enumerate(batches):
        step(sk, se, lb)
        tstep.forward_backward(sk, se, tstep.prepare(sk, se, lb))
        assert torch.equal(bits(step.loss), bits(tstep.loss))
        exp = tstep.grads.clone() if fresh else exp.add_(tstep.grads)
        fresh = False
        if due[i]:
            tstep.grads.copy_(exp)
            tstep.optimizer_step()
            fresh = True
        torch.cuda.synchronize()
        _same_state(model, twin)
        assert torch.equal(bits(step.accum), bits(exp)), i
    assert step.steps_taken() == 3


def test_captured_step_follows_a_change_of_the_weights(state, batches):
    """Four steps, captured and eager, with step.class_weight = w2 after the second on both: the same losses,
    parameters and square_avg, bit for bit. The launch reads the device array when it is replayed."""
    import fall_multimodal_amd as f3
    d = dev()
    w1, w2 = _weights(7), _weights(8)
    runs = []
    for captured in (False, True):
        model = _net(d, state)
        step = f3.TrainStep(model, B, lr=1e-3, class_weight=w1)
        if captured:
            sk, se, lb = (t.clone() for t in batches[0])
            step.capture(sk, se, step.prepare(sk, se, lb))
        losses = []
        for i, (sk, se, lb) in enumerate(batches):
            if i == 2:
                step.class_weight = w2
                np.testing.assert_array_equal(step.class_weight.cpu().numpy(), w2)
            losses.append(step(sk, se, lb).clone())
        torch.cuda.synchronize()
        runs.append((step, losses))
    (eager, le), (graph, lg) = runs
    for a, b in zip(le, lg):
        assert torch.equal(bits(a), bits(b)), (float(a.item()), float(b.item()))
    assert torch.equal(eager.model.flat_parameters(), graph.model.flat_parameters())
    assert torch.equal(eager.square_avg, graph.square_avg)
    # the change took effect: the third loss is f3_soft_ce_w's with w2 on the step's own output
    sk, se, lb = batches[3]
    loss_t, _ = weighted(d, graph.out.cpu().numpy(), lb.cpu().numpy(), w2, 0.0)
    assert torch.equal(bits(lg[3]), bits(loss_t))
    loss_old, _ = weighted(d, graph.out.cpu().numpy(), lb.cpu().numpy(), w1, 0.0)
    assert not torch.equal(bits(lg[3]), bits(loss_old))


def test_weights_cannot_be_added_or_removed_later(state):
    import fall_multimodal_amd as f3
    d = dev()
    plain = f3.TrainStep(_net(d, state), B)
    with pytest.raises(ValueError, match="class_weight"):
        plain.class_weight = np.ones(11)
    step = f3.TrainStep(_net(d, state), B, class_weight=np.ones(11))
    with pytest.raises(ValueError, match="class_weight"):
        step.class_weight = None
    for bad in (np.ones(10), -np.ones(11), np.zeros(11)):
        with pytest.raises(ValueError):
            step.class_weight = bad
        with pytest.raises(ValueError):
            f3.TrainStep(_net(d, state), B, class_weight=bad)
    assert step.class_weight.tolist() == [1.0] * 11  # a refused value changes nothing
    step.class_weight.fill_(3.0)                     # the property hands out a copy
    assert step.class_weight.tolist() == [1.0] * 11


# ---- 7. the side steps (B = 4, V = 14: the shapes of their golden fixtures) --------------------------------
def _side(kind, d, **kw):
    """(step, x, label, extra call arguments) on a freshly initialised model."""
    import fall_multimodal_amd as f3
    if kind == "targcn":
        from oracle import targcn_cpu as tg
        model = f3.TARGCN(num_nodes=14, device=d)
        model.load_state_dict(tg.init_state(14, 11))
        x, label = tg.synthetic_source(4, 14, 11, 5)
        return f3.TargcnStep(model, 4, lr=1e-5, **kw), x, label, {}
    if kind == "sktr":
        from oracle import sktr_cpu as sk
        model = f3.SkeletonTransformer(device=d)
        model.load_state_dict(sk.init_state(31))
        x, label = sk.synthetic_clips(4, 14, 11, 77)
        sd = [1.0, 1.0, 1.0, 0.0, 1.25, 1.25, 1.5, 1.5, 0.0, 2.0, 0.0, 2.0, 1.0 / 0.6, 1.0 / 0.6, 1.0 / 0.6, 0.0, 2.0, 2.0]
        return f3.SktrStep(model, 4, **kw), x, label, dict(sd=sd, seed=12345)
    from oracle import musa_cpu as mu
    model = f3.musa.Model(11, 14, 300, f3.musa.adjGraph("coco_cut", "uniform"), True, True, 41, device=d)
    model.load_state_dict(mu.init_state(77), strict=True)
    x, _, label = synthetic_batch(4, 14, 11, 1, 123)
    return f3.musa.MusaStep(model, 4, **kw), x, label, dict(seed=4242)


_SIDE_ONES = {}


def _side_ones_run(kind):
    """Two steps of a side step built with all-ones weights, run once per model and shared. After each, the
    default step's loss launch (f3_soft_ce) is run by hand on the step's own `out`: the loss word and dout
    of the two launches. The side models' backward passes (and musa's forward) add with float atomics, so two
    default steps do not reproduce each other's gradients bit for bit; the loss launch is what changes, and
    everything downstream consumes its dout, so the comparison is made there, on identical inputs."""
    if kind not in _SIDE_ONES:
        from fall_multimodal_amd._lib import lib, ptr, stream_handle
        d = dev()
        ones, x, label, extra = _side(kind, d, class_weight=np.ones(11))
        x_t, label_t = torch.from_numpy(x).to(d), torch.from_numpy(label).to(d)
        rec = {"loss": [], "dout": []}
        for _ in range(2):
            ones(x_t, label_t, **extra)
            loss0, dout0 = nan_pair(d, 4, 11)
            assert lib().f3_soft_ce(ptr(ones.out), ptr(label_t), 4, 11, ptr(loss0), ptr(dout0), stream_handle()) == 0
            rec["loss"].append((int(bits(ones.loss).item()), int(bits(loss0).item())))
            rec["dout"].append(torch.equal(bits(ones.dout), bits(dout0)))
        torch.cuda.synchronize()
        assert np.isfinite(float(ones.loss.item())) and bool(ones.grads.any())
        _SIDE_ONES[kind] = rec
    return _SIDE_ONES[kind]


@pytest.mark.parametrize("kind", ["targcn", "sktr", "musa"])
def test_side_steps_all_ones_weights_give_the_default_dout(kind):
    rec = _side_ones_run(kind)
    assert rec["dout"] == [True, True], rec


@pytest.mark.parametrize("kind", ["targcn", "sktr", "musa"])
def test_side_steps_all_ones_weights_log_the_default_loss(kind):
    """The loss word beside f3_soft_ce's on the same `out`, both steps."""
    rec = _side_ones_run(kind)
    print(f"{kind}: loss words (all-ones weights, f3_soft_ce) per step {rec['loss']}")
    assert all(a == b for a, b in rec["loss"]), rec["loss"]


@pytest.mark.parametrize("kind", ["targcn", "sktr", "musa"])
def test_side_steps_take_class_weights(kind):
    """Random weights: the loss and dout bits of f3_soft_ce_w (eps 0) on the step's own out; a default step has
    no weights; a wrong length is refused."""
    d = dev()
    w = _weights(9)
    step, x, label, extra = _side(kind, d, class_weight=w)
    x_t, label_t = torch.from_numpy(x).to(d), torch.from_numpy(label).to(d)
    np.testing.assert_array_equal(step.class_weight.cpu().numpy(), w)
    for _ in range(2):
        step(x_t, label_t, **extra)
        torch.cuda.synchronize()
        out = step.out.cpu().numpy()
        loss_t, dout_t = weighted(d, out, label, w, 0.0)
        assert torch.equal(bits(step.loss), bits(loss_t)) and torch.equal(bits(step.dout), bits(dout_t))
        rl, rd = R.gate_ratios(float(step.loss.item()), step.dout.cpu().numpy(), out, label, w, 0.0)
        assert rl <= 1.0 and rd <= 1.0, (kind, rl, rd)
    plain = _side(kind, d)[0]
    assert plain.class_weight is None
    with pytest.raises(ValueError):
        _side(kind, d, class_weight=np.ones(10))


# ---- 8. the eval loops --------------------------------------------------------------------------------
def test_eval_loops_take_class_weights_under_both_rules():
    """80 windows in batches of 32, 32 and 16. 2-D labels: torch's rule for probability targets; 1-D labels
    (their argmax): its rule for class indices. Each is the mean of the per-batch fp64 torch losses of the
    model's own outputs, within the loss gate (the mean of the per-batch bounds); the two differ."""
    import fall_multimodal_amd as f3
    from fall_multimodal_amd import evaluate as fe
    d = dev()
    model = f3.TwoStreamSTGCAN_BiLSTM(3, {"layout": "coco_mmpose", "strategy": "spatial"}, 11, 6, device=d)
    model.load_state_dict(oc.init_state(SPEC, 31))
    model.train()
    with torch.no_grad():  # one train-mode forward moves the BN running statistics
        model(*(torch.from_numpy(x).to(d) for x in synthetic_batch(64, 18, 11, 6, 20)[:2]))
    skel, sensor, label = synthetic_batch(80, 18, 11, 6, 21)
    w = _weights(10)
    eps = 0.1
    cuts = [(0, 32), (32, 64), (64, 80)]
    results = {}
    for form in ("soft", "index"):
        lab = label if form == "soft" else label.argmax(1).astype(np.int64)
        loader = [tuple(torch.from_numpy(np.ascontiguousarray(a[lo:hi])).to(d) for a in (skel, sensor, lab))
                  for lo, hi in cuts]
        got = fe.valid_device(model, loader, top_k=(1, 5), class_weight=w, label_smoothing=eps)
        model.eval()
        want, bound = [], []
        with torch.no_grad():
            for sk_t, se_t, _ in loader:
                out = model(sk_t, se_t).cpu().numpy()
                lo = cuts[len(want)][0]
                lb = lab[lo:lo + out.shape[0]]
                wl, _ = R.torch_reference(out, lb, w, eps)
                m, D = R.scales(lb, w, eps, 11)
                want.append(wl)
                bound.append(R.LOSS_TOL["atol"] * max(1.0, m.sum() / D) + R.LOSS_TOL["rtol"] * abs(wl))
        model.train()
        print(f"{form}: valid_device weighted loss {got['loss']!r}, fp64 torch {float(np.mean(want))!r}")
        assert abs(got["loss"] - float(np.mean(want))) <= float(np.mean(bound)), (form, got["loss"], want)
        tst = fe.test_device(model, loader, top_k=(1, 5), class_weight=w, label_smoothing=eps)
        assert tst["loss"] == got["loss"] and tst["top_k"] == got["top_k"]
        plain = fe.valid_device(model, loader, top_k=(1, 5), label_smoothing=eps)
        assert plain["top_k"] == got["top_k"] and abs(plain["loss"] - got["loss"]) > 1e-3
        results[form] = got["loss"]
    assert abs(results["soft"] - results["index"]) > 1e-3  # the index rule divides by W, not N
    with pytest.raises(ValueError):
        fe.valid_device(model, loader, class_weight=np.ones(10))
    assert model.training
