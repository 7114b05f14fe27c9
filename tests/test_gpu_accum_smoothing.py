"""Label smoothing and gradient accumulation on the MI355X: f3_soft_ce_ex against fp64 numpy and
against f3_soft_ce's bits at eps = 0, f3_grad_accumulate against torch bit for bit, the
accumulating TrainStep (eager and captured) against a twin step driven by hand, the defaults
against today's step, smoothing inside the step and the eval loops, and two data-parallel ranks
(tools/accum_dp_check.py).

The rule (include/fall3.h, torch.nn.CrossEntropyLoss(label_smoothing=eps) for probability targets,
applied to class indices as one-hot rows): y' = y (1 - eps) + eps / C,
loss = -(1/N) sum_n sum_c y'_c log_softmax(out)_c, dout = (softmax(out) sum_c y'_c - y') / N."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import model_cpu as oc
from oracle.prng import synthetic_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORM_RTOL = 2.0 ** -22                 # fp64 sum rounded to fp32 once (tests/test_gpu_metrics.py)
LOSS_TOL = dict(rtol=1e-5, atol=2e-5)  # fp32 expf / logf / subtraction per row: a few ulp of |lse| <= ~13
# |d dout| N / max(1, sum_c y'_c): one ulp of |lse| <= 13 in o - lse is ~1e-6 relative in expf; an fp32
# emulation of the kernel's sums reached 4.0e-7, and the device's expf / logf may differ from numpy's
# by a few ulp: a factor of five
DOUT_TOL = 2e-6
EINVAL = 1001
B = 8


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda")


# ---- the host reference ---------------------------------------------------------------------------
def smoothed(label, C, eps):
    """y' in fp64; an index label is one-hot."""
    if label.ndim == 1:
        y = np.zeros((label.shape[0], C))
        y[np.arange(label.shape[0]), label] = 1.0
    else:
        y = label.astype(np.float64)
    return y * (1.0 - eps) + eps / C


def soft_ce_ex(out, label, eps):
    """tests/test_gpu_metrics.py's soft_ce extended with y': (loss, dout, sum_c y'_c per row), fp64."""
    o = out.astype(np.float64)
    N, C = o.shape
    y = smoothed(label, C, eps)
    mx = o.max(1, keepdims=True)
    lsm = o - (mx + np.log(np.exp(o - mx).sum(1, keepdims=True)))
    ys = y.sum(1, keepdims=True)
    return float(-(y * lsm).sum(1).mean()), (np.exp(lsm) * ys - y) / N, ys[:, 0]


def gate_ratios(loss, dout, out, label, eps):
    """(loss gate used, dout gate used), each as a fraction of its bound (<= 1 passes)."""
    want_l, want_d, ys = soft_ce_ex(out, label, eps)
    rl = abs(loss - want_l) / (LOSS_TOL["atol"] + LOSS_TOL["rtol"] * abs(want_l))
    rd = 0.0
    if dout is not None:
        N = out.shape[0]
        rd = float((np.abs(dout.astype(np.float64) - want_d) * N / np.maximum(1.0, ys)[:, None]).max()) / DOUT_TOL
    return rl, rd


def make_case(rng, N, C, form):
    out = rng.uniform(-4.0, 4.0, (N, C)).astype(np.float32)
    if form == "index":
        return out, rng.integers(0, C, N).astype(np.int64)
    label = rng.random((N, C)).astype(np.float32)
    label /= label.sum(1, keepdims=True)
    if form == "soft075":  # rows that do not sum to 1: nothing renormalises them
        label = (label * np.float32(0.75)).astype(np.float32)
    return out, label


def run_sce(out_t, label_t, eps, loss_t, dout_t, N=None, C=None, both=None):
    """f3_soft_ce_ex's status; a 2-D label is the soft form, a 1-D one the index form."""
    from fall_multimodal_amd._lib import lib, ptr, stream_handle
    soft, idx = (label_t, None) if (label_t is not None and label_t.dim() == 2) else (None, label_t)
    if both is not None:
        soft, idx = both
    return lib().f3_soft_ce_ex(ptr(out_t), ptr(soft), ptr(idx), out_t.shape[0] if N is None else N,
                               out_t.shape[1] if C is None else C, eps, ptr(loss_t), ptr(dout_t), stream_handle())


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. the loss kernel against fp64 --------------------------------------------------------------
@pytest.mark.parametrize("form", ["soft", "soft075", "index"])
@pytest.mark.parametrize("C", [2, 11, 17, 64])
def test_soft_ce_ex_matches_fp64(C, form):
    """N in {1, 63, 64, 65, 257, 300} (one thread, a wave and its neighbours, more than one pass of the
    workgroup) x eps in {0.1, 1.0}; C = 2, 11 take the register path, 17, 64 the row-in-memory path.
    dout = NULL gives the same loss bits and writes nothing around the loss word."""
    d = dev()
    worst_l = worst_d = 0.0
    for N in (1, 63, 64, 65, 257, 300):
        for eps in (0.1, 1.0):
            rng = np.random.default_rng(100000 * C + 100 * N + int(10 * eps))
            out, label = make_case(rng, N, C, form)
            out_t, label_t = torch.from_numpy(out).to(d), torch.from_numpy(label).to(d)
            loss_t = torch.full((1,), float("nan"), device=d)
            dout_t = torch.full((N, C), float("nan"), device=d)
            assert run_sce(out_t, label_t, eps, loss_t, dout_t) == 0
            loss, dout = float(loss_t.cpu()[0]), dout_t.cpu().numpy()
            assert np.isfinite(loss) and np.isfinite(dout).all()
            rl, rd = gate_ratios(loss, dout, out, label, eps)
            worst_l, worst_d = max(worst_l, rl), max(worst_d, rd)
            assert rl <= 1.0, (N, C, eps, form, loss, rl)
            assert rd <= 1.0, (N, C, eps, form, rd)
            # loss only: a sentinel-filled buffer around the loss word stays as it was
            guard = torch.full((129,), -7.5, device=d)
            assert run_sce(out_t, label_t, eps, guard[64:65], None) == 0
            assert torch.equal(bits(guard[64:65]), bits(loss_t)), (N, C, eps, form)
            rest = torch.cat([guard[:64], guard[65:]])
            assert bool((rest == -7.5).all()), (N, C, eps, form)
            assert torch.equal(out_t.cpu(), torch.from_numpy(out))  # the inputs are only read
    print(f"C={C} {form}: worst loss gate ratio {worst_l:.4f}, worst dout gate ratio {worst_d:.4f}")


# ---- 2. eps = 0 is f3_soft_ce ---------------------------------------------------------------------
@pytest.mark.parametrize("C", [11, 17])
@pytest.mark.parametrize("N", [8, 300])
def test_eps_zero_reproduces_soft_ce_bit_for_bit(N, C):
    from fall_multimodal_amd._lib import lib, ptr, stream_handle
    d = dev()
    out, label = make_case(np.random.default_rng(5 + N + C), N, C, "soft")
    out_t, label_t = torch.from_numpy(out).to(d), torch.from_numpy(label).to(d)
    loss0, dout0 = torch.full((1,), float("nan"), device=d), torch.full((N, C), float("nan"), device=d)
    assert lib().f3_soft_ce(ptr(out_t), ptr(label_t), N, C, ptr(loss0), ptr(dout0), stream_handle()) == 0
    runs = []
    for _ in range(2):
        loss1, dout1 = torch.full((1,), float("nan"), device=d), torch.full((N, C), float("nan"), device=d)
        assert run_sce(out_t, label_t, 0.0, loss1, dout1) == 0
        runs.append((loss1, dout1))
    assert np.isfinite(float(loss0.cpu()[0]))
    for loss1, dout1 in runs:
        assert torch.equal(bits(loss1), bits(loss0)), (float(loss1.cpu()[0]), float(loss0.cpu()[0]))
        assert torch.equal(bits(dout1), bits(dout0))


@pytest.mark.parametrize("C", [11, 17])
def test_large_batch_path_is_reproducible_and_inside_the_gate(C):
    """N = 5000 > 4096: per-workgroup partials added in index order."""
    d = dev()
    N = 5000
    for form, eps in (("soft", 0.0), ("soft", 0.1), ("index", 0.1)):
        out, label = make_case(np.random.default_rng(77 + C), N, C, form)
        out_t, label_t = torch.from_numpy(out).to(d), torch.from_numpy(label).to(d)
        runs = []
        for _ in range(2):
            loss_t, dout_t = torch.full((1,), float("nan"), device=d), torch.full((N, C), float("nan"), device=d)
            assert run_sce(out_t, label_t, eps, loss_t, dout_t) == 0
            runs.append((loss_t, dout_t))
        assert torch.equal(bits(runs[0][0]), bits(runs[1][0])) and torch.equal(bits(runs[0][1]), bits(runs[1][1]))
        rl, rd = gate_ratios(float(runs[0][0].cpu()[0]), runs[0][1].cpu().numpy(), out, label, eps)
        print(f"N={N} C={C} {form} eps={eps}: loss gate ratio {rl:.4f}, dout gate ratio {rd:.4f}")
        assert rl <= 1.0 and rd <= 1.0, (rl, rd)
        only = torch.full((1,), float("nan"), device=d)
        assert run_sce(out_t, label_t, eps, only, None) == 0
        assert torch.equal(bits(only), bits(runs[0][0]))


# ---- 3. refusals ----------------------------------------------------------------------------------
def test_soft_ce_ex_refuses_bad_arguments():
    d = dev()
    out_t = torch.zeros(4, 11, device=d)
    soft = torch.full((4, 11), 1.0 / 11, device=d)
    idx = torch.zeros(4, dtype=torch.int64, device=d)
    loss_t, dout_t = torch.full((1,), -7.5, device=d), torch.full((4, 11), -7.5, device=d)
    for eps in (-0.1, 1.5, float("nan"), float("inf")):
        assert run_sce(out_t, soft, eps, loss_t, dout_t) == EINVAL, eps
    assert run_sce(out_t, None, 0.1, loss_t, dout_t, both=(soft, idx)) == EINVAL
    assert run_sce(out_t, None, 0.1, loss_t, dout_t, both=(None, None)) == EINVAL
    wide = torch.zeros(4, 65, device=d)
    assert run_sce(wide, torch.zeros(4, 65, device=d), 0.1, loss_t, torch.zeros(4, 65, device=d)) == EINVAL
    assert run_sce(out_t, soft, 0.1, loss_t, dout_t, N=0) == EINVAL
    assert run_sce(out_t, soft, 0.1, loss_t, dout_t, C=0) == EINVAL
    torch.cuda.synchronize()
    assert float(loss_t.cpu()[0]) == -7.5 and bool((dout_t == -7.5).all())  # a refused call launches nothing
    assert run_sce(out_t, soft, 0.1, loss_t, dout_t) == 0 and run_sce(out_t, idx, 1.0, loss_t, dout_t) == 0


# ---- 4. f3_grad_accumulate ------------------------------------------------------------------------
def _accumulate(acc, g, flag, n=None):
    from fall_multimodal_amd._lib import lib, ptr, stream_handle
    return lib().f3_grad_accumulate(ptr(acc), ptr(g), g.numel() if n is None else n, ptr(flag), stream_handle())


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1023, 1024, 1025, 4 * 256 * 4096 + 7])
def test_grad_accumulate_copies_then_adds_bit_for_bit(n):
    """The last n is more than one grid-stride pass of the capped grid plus a tail."""
    d = dev()
    rng = np.random.default_rng(n % 9973)
    special = np.array([0x80000000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0x00000001, 0x7F800000], dtype=np.uint32)
    g_bits = rng.standard_normal(n).astype(np.float32).view(np.uint32).copy()
    k = min(n, special.size)
    g_bits[:k] = special[:k]  # -0.0, NaN payloads, a denormal, inf
    if n > 8:
        g_bits[-3:] = special[:3]  # and in the scalar tail
    g = torch.from_numpy(g_bits.view(np.int32)).to(d).view(torch.float32)
    acc = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(d)  # values already there
    flag = torch.ones(1, dtype=torch.int32, device=d)
    assert _accumulate(acc, g, flag) == 0
    assert int(flag.cpu()[0]) == 0
    assert torch.equal(bits(acc), bits(g))                                   # flag 1: a bitwise copy
    g1_host = torch.from_numpy(rng.standard_normal(n).astype(np.float32))
    g1 = g1_host.to(d)
    g2 = torch.from_numpy((rng.standard_normal(n) * 1e-3).astype(np.float32)).to(d)
    flag.fill_(1)
    assert _accumulate(acc, g1, flag) == 0
    assert int(flag.cpu()[0]) == 0
    want = g1 + g2
    assert _accumulate(acc, g2, flag) == 0                                   # flag 0: one fp32 add
    assert int(flag.cpu()[0]) == 0
    assert torch.equal(bits(acc), bits(want))
    want = want + g1
    assert _accumulate(acc, g1, flag) == 0
    assert torch.equal(bits(acc), bits(want)) and int(flag.cpu()[0]) == 0
    assert torch.equal(g1.cpu(), g1_host) and acc.numel() == n  # the gradient is only read


def test_grad_accumulate_refuses_misaligned_pointers():
    d = dev()
    buf, g = torch.zeros(16, device=d), torch.ones(16, device=d)
    flag = torch.ones(1, dtype=torch.int32, device=d)
    assert _accumulate(buf[1:9], g[:8], flag) == EINVAL
    assert _accumulate(buf[:8], g[1:9], flag) == EINVAL
    assert _accumulate(buf, g, flag, n=-1) == EINVAL
    assert _accumulate(buf, g, None) == EINVAL
    torch.cuda.synchronize()
    assert int(flag.cpu()[0]) == 1 and not bool(buf.any())  # a refused call changes nothing
    assert _accumulate(buf[4:12], g[4:12], flag) == 0 and int(flag.cpu()[0]) == 0
    assert buf.cpu().tolist() == [0.0] * 4 + [1.0] * 8 + [0.0] * 4


# ---- the model ------------------------------------------------------------------------------------
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
    return [[torch.from_numpy(x).to(d) for x in synthetic_batch(B, 18, 11, 6, 70 + i)] for i in range(5)]


def _pair(d, st, opt, **kw):
    """An accumulating (or otherwise configured) step and a plain twin from the same state."""
    import fall_multimodal_amd as f3
    model, twin = _net(d, st), _net(d, st)
    if opt == "sgd_clip":
        # the summed gradients' norm is far above 0.05: the update is clipped (asserted by the caller)
        step = f3.TrainStep(model, B, optimizer=f3.SGD(model.parameters(), lr=1e-3), max_norm=0.05, **kw)
        tstep = f3.TrainStep(twin, B, optimizer=f3.SGD(twin.parameters(), lr=1e-3), max_norm=0.05)
    else:
        step, tstep = f3.TrainStep(model, B, lr=1e-3, **kw), f3.TrainStep(twin, B, lr=1e-3)
    return model, twin, step, tstep


def _same_state(model, twin):
    assert torch.equal(model.flat_parameters(), twin.flat_parameters())
    assert torch.equal(model._flat_buffers, twin._flat_buffers)


def _twin_grad(tstep, sk, se, lb):
    tstep.forward_backward(sk, se, tstep.prepare(sk, se, lb))
    return tstep.grads


# ---- 5. the accumulating step against a twin --------------------------------------------------------
@pytest.mark.parametrize("opt", ["rmsprop", "sgd_clip"])
@pytest.mark.parametrize("mode", ["eager", "captured"])
def test_accumulating_step_matches_a_twin_driven_by_hand(mode, opt, state, batches):
    """accum_iter = 3, five batches after begin_epoch(5): updates after batches 0, 3 and 4. The twin
    runs forward_backward per batch, the test folds its gradients (exp = g after an update, exp += g
    otherwise: autograd's order) and feeds the sum to the twin's flat update on update batches. After
    every batch the parameters, the BN buffers, accum and pending agree bit for bit."""
    from fall_multimodal_amd.train import accum_updates
    d = dev()
    model, twin, step, tstep = _pair(d, state, opt, accum_iter=3)
    assert step.accum is not None and step.accum.numel() == step.grads.numel() and step.pending == 0
    if mode == "captured":
        for s in (step, tstep):  # (the twin for capture()'s warm-up forwards, which move the BN statistics)
            s.capture(*(t.clone() for t in batches[0]))
        assert step.pending == 0
    due = accum_updates(5, 3)
    assert due == [True, False, False, True, True]
    step.begin_epoch(5)
    exp, fresh, pend = None, True, 0
    for i, (sk, se, lb) in enumerate(batches):
        step(sk, se, lb)
        g = _twin_grad(tstep, sk, se, lb)
        if fresh:
            exp = g.clone()
        else:
            exp += g
        fresh, pend = False, pend + 1
        if due[i]:
            tstep.grads.copy_(exp)
            tstep.optimizer_step()
            fresh, pend = True, 0
        torch.cuda.synchronize()
        _same_state(model, twin)
        assert torch.equal(bits(step.accum), bits(exp)), i
        assert step.pending == pend, (i, step.pending, pend)
        if due[i] and opt == "sgd_clip":
            assert 0.0 < float(step.clip_coef.item()) < 1.0
            assert torch.equal(step.grad_norm, tstep.grad_norm) and torch.equal(step.clip_coef, tstep.clip_coef)
    assert step.steps_taken() == 3 and tstep.steps_taken() == 3
    sd = step.optimizer_state_dict()
    assert {int(v["step"]) for v in sd["state"].values() if "step" in v} <= {3}  # updates, not micro-batches
    # the reports show what the update consumed: accum
    base = step.accum.untyped_storage().data_ptr()
    names, norms = step.param_grad_norms()
    got = norms.cpu().numpy().astype(np.float64)
    total = 0.0
    for (n, p), gn in zip(model.named_parameters(), got):
        assert p.grad.untyped_storage().data_ptr() == base, n
        w = float(p.grad.double().norm().item())
        total += float((p.grad.double() ** 2).sum().item())
        assert abs(gn - w) <= NORM_RTOL * w, (n, gn, w)
    assert names == [n for n, _ in model.named_parameters()]
    assert total > 0 and abs(got[-1] - np.sqrt(total)) <= NORM_RTOL * np.sqrt(total)


# ---- 6. update= and zero_grad() --------------------------------------------------------------------
def test_update_argument_and_zero_grad(state, batches):
    """zero_grad() after two micro-batches makes the next one overwrite; update=False, False, True is
    one twin update on the sum of three; update=False three times and then True one on the sum of
    four (the updating call is a micro-batch too)."""
    d = dev()
    model, twin, step, tstep = _pair(d, state, "rmsprop", accum_iter=3)
    b = batches
    for sk, se, lb in b[:2]:
        step(sk, se, lb, update=False)
        _twin_grad(tstep, sk, se, lb)
    assert step.pending == 2
    step.zero_grad()
    assert step.pending == 0
    step(*b[2], update=False)
    g = _twin_grad(tstep, *b[2])
    torch.cuda.synchronize()
    assert step.pending == 1 and torch.equal(bits(step.accum), bits(g))
    _same_state(model, twin)  # nothing has updated yet
    assert step.steps_taken() == 0
    step.zero_grad()
    for window in (b[:3], b[1:5]):
        exp = None
        for j, (sk, se, lb) in enumerate(window):
            last = j == len(window) - 1
            step(sk, se, lb, update=last)
            g = _twin_grad(tstep, sk, se, lb)
            exp = g.clone() if exp is None else exp.add_(g)
            assert step.pending == (0 if last else j + 1)
        tstep.grads.copy_(exp)
        tstep.optimizer_step()
        torch.cuda.synchronize()
        assert torch.equal(bits(step.accum), bits(exp))
        _same_state(model, twin)
    assert step.steps_taken() == 2
    plain = _pair(d, state, "rmsprop")[2]
    with pytest.raises(ValueError, match="accum_iter"):
        plain(*b[0], update=False)
    with pytest.raises(ValueError, match="accum_iter"):
        plain.zero_grad()


# ---- 7. the defaults are today's step ------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eager", "captured"])
def test_defaults_are_todays_step(mode, state, batches):
    import fall_multimodal_amd as f3
    d = dev()
    model, twin = _net(d, state), _net(d, state)
    step = f3.TrainStep(model, B, label_smoothing=0.0, accum_iter=1)
    tstep = f3.TrainStep(twin, B)
    assert not hasattr(step, "accum") or step.accum is None
    assert step.fused_optimizer == tstep.fused_optimizer and step.phased == tstep.phased
    if mode == "captured":
        for s in (step, tstep):
            s.capture(*(t.clone() for t in batches[0]))
    for sk, se, lb in batches[:2]:
        step(sk, se, lb)
        tstep(sk, se, lb)
    torch.cuda.synchronize()
    _same_state(model, twin)
    assert torch.equal(bits(step.grads), bits(tstep.grads)) and torch.equal(bits(step.loss), bits(tstep.loss))
    assert step.steps_taken() == 2
    for p, q in zip(model.parameters(), twin.parameters()):
        assert p.grad.untyped_storage().data_ptr() == step.grads.untyped_storage().data_ptr()
        assert torch.equal(p.grad, q.grad)


# ---- 8. smoothing in the step and in the eval loops --------------------------------------------------------
@pytest.mark.parametrize("mode", ["eager", "captured"])
def test_step_uses_the_smoothed_loss(mode, state, batches):
    import fall_multimodal_amd as f3
    d = dev()
    eps = 0.1
    model = _net(d, state)
    step = f3.TrainStep(model, B, lr=1e-3, label_smoothing=eps, metrics=True)
    if mode == "captured":
        step.capture(*(t.clone() for t in batches[0]))
    loss_sum = np.float64(0.0)
    plain = []
    for sk, se, lb in batches[:3]:
        step(sk, se, lb)
        torch.cuda.synchronize()
        out, label = step.out.cpu().numpy(), lb.cpu().numpy()
        loss = step.loss.cpu().numpy()[0]
        rl, rd = gate_ratios(float(loss), step.dout.cpu().numpy(), out, label, eps)
        print(f"{mode}: step loss {float(loss)!r}, loss gate ratio {rl:.4f}, dout gate ratio {rd:.4f}")
        assert rl <= 1.0 and rd <= 1.0, (rl, rd)
        plain.append(soft_ce_ex(out, label, 0.0)[0])
        assert abs(float(loss) - plain[-1]) > 1e-3  # it is not the unsmoothed loss
        loss_sum = loss_sum + np.float64(loss)
    blk = step.metrics.block.cpu().numpy()
    assert int(blk[1]) == 3 and int(blk[2]) == 3 * B
    assert blk[0:1].view(np.float64)[0].tobytes() == loss_sum.tobytes()  # the smoothed loss is what is logged
    # ranks and confusion come from the unsmoothed label: every row counted once, on its true class's row
    conf = blk[11:].reshape(11, 11)
    true = np.concatenate([lb.cpu().numpy().argmax(1) for _, _, lb in batches[:3]])
    np.testing.assert_array_equal(conf.sum(1), np.bincount(true, minlength=11))


def test_eval_loops_take_label_smoothing():
    """80 windows behind a batch-32 loader (last batch 16), as tests/test_gpu_metrics.py."""
    import fall_multimodal_amd as f3
    from fall_multimodal_amd import data as fd
    from fall_multimodal_amd import evaluate as fe
    d = dev()
    model = f3.TwoStreamSTGCAN_BiLSTM(3, {"layout": "coco_mmpose", "strategy": "spatial"}, 11, 6, device=d)
    model.load_state_dict(oc.init_state(SPEC, 31))
    model.train()
    with torch.no_grad():  # one train-mode forward moves the BN running statistics
        model(*(torch.from_numpy(x).to(d) for x in synthetic_batch(64, 18, 11, 6, 20)[:2]))
    skel, sensor, label = synthetic_batch(80, 18, 11, 6, 21)
    w = fd.Windows([f"v{i // 4}" for i in range(80)], np.ascontiguousarray(skel.transpose(0, 2, 3, 1)), sensor, label)
    loader = fd.WindowLoader(w, 32, shuffle=False, drop_last=False, device=d)
    got = fe.valid_device(model, loader, top_k=(1, 5), label_smoothing=0.1)
    want = fe.valid(model, loader, torch.nn.CrossEntropyLoss(label_smoothing=0.1), top_k=(1, 5))
    print(f"valid_device smoothed loss {got['loss']!r}, evaluate.valid {want['loss']!r}")
    np.testing.assert_allclose(got["loss"], want["loss"], **LOSS_TOL)
    assert got["top_k"] == want["top_k"]
    plain = fe.valid_device(model, loader, top_k=(1, 5))
    assert plain["top_k"] == got["top_k"] and abs(plain["loss"] - got["loss"]) > 1e-3
    tst = fe.test_device(model, loader, top_k=(1, 5), label_smoothing=0.1)
    assert tst["loss"] == got["loss"] and tst["top_k"] == got["top_k"]
    assert tst["confusion"] == fe.test_device(model, loader, top_k=(1, 5))["confusion"]
    with pytest.raises(ValueError, match="label_smoothing"):
        fe.valid_device(model, loader, label_smoothing=1.5)
    assert model.training


# ---- 9. two ranks ---------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_reduce_only_on_update_calls():
    dev()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "tools", "accum_dp_check.py"),
           "--backend", "gloo", "--same-device"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and lines, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(lines[-1])
    print(res)
    assert res["world"] == 2 and res["replicas_identical"] and res["max_param_change"] > 0
    assert res["all_reduce_rounds"] == 3 and res["all_reduce_calls"] == 6
    assert res["window_sum_bitwise"] is True and res["pending_ok"] and res["steps_taken"] == 3
