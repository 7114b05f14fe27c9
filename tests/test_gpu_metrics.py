"""Device-side step metrics on the MI355X: f3_metrics_update's counts and loss, f3_segment_norms,
their use inside TrainStep (eager and captured) and evaluate.valid_device / test_device.
References are numpy / fp64 on the host, computed from the same device tensors copied back.

The rule under test (include/fall3.h): the true class is the first arg-max of the soft label (or
the given index), the predicted class the first arg-max of the logits, the target's rank the number
of classes c with out[c] > out[t], or out[c] == out[t] and c < t, a NaN logit ordering above every
number; correct[j] counts the rows with rank < top_k[j]."""
import numpy as np
import pytest
import torch

from oracle import model_cpu as oc
from oracle.prng import synthetic_batch

pytestmark = pytest.mark.gpu

NORM_RTOL = 2.0 ** -22      # fp64 sum rounded to fp32 once (tests/test_gpu_optim.py)
LOSS_TOL = dict(rtol=1e-5, atol=2e-5)  # fp32 expf / logf / subtraction per row: a few ulp of |lse| <= ~13


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda")


# ---- the host reference ---------------------------------------------------------------------------
def _ahead(out, ref, ref_idx):
    """[N,C] bool: class c precedes the class ref_idx (whose logit is ref) in the stated order."""
    x, r = out, ref[:, None]
    xn, rn = np.isnan(x), np.isnan(r)
    with np.errstate(invalid="ignore"):
        gt = (x > r) | (xn & ~rn)
        eq = (x == r) | (xn & rn)
    return gt | (eq & (np.arange(out.shape[1])[None, :] < ref_idx[:, None]))


def ref_counts(out, true, top_k):
    """(rank of the target per row, predicted class per row) by the stated rule."""
    N, C = out.shape
    rows = np.arange(N)
    rank = _ahead(out, out[rows, true], true).sum(1)
    pred = np.full(N, -1)
    for c in range(C):  # the prediction is the one class nothing precedes
        cc = np.full(N, c)
        pred[_ahead(out, out[:, c], cc).sum(1) == 0] = c
    assert (pred >= 0).all()
    if not np.isnan(out).any():
        assert (pred == np.argmax(out, 1)).all()  # first-occurrence arg-max
    return rank, pred


class Ref:
    """Accumulates what the device block should hold."""

    def __init__(self, C, top_k):
        self.C, self.top_k = C, top_k
        self.batches = self.rows = 0
        self.correct = np.zeros(8, dtype=np.int64)
        self.confusion = np.zeros((C, C), dtype=np.int64)

    def add(self, out, label):
        true = label if label.ndim == 1 else np.argmax(label, 1)
        rank, pred = ref_counts(out, true, self.top_k)
        self.batches += 1
        self.rows += out.shape[0]
        for j, k in enumerate(self.top_k):
            self.correct[j] += int((rank < k).sum())
        np.add.at(self.confusion, (true, pred), 1)


def read_block(m):
    blk = m.block.cpu().numpy()
    C = m.num_class
    return {"loss_sum": blk[0:1].view(np.float64)[0], "batches": int(blk[1]), "rows": int(blk[2]),
            "correct": blk[3:11].copy(), "confusion": blk[11:].reshape(C, C).copy()}


def assert_counts(m, ref, what=""):
    got = read_block(m)
    assert got["batches"] == ref.batches and got["rows"] == ref.rows, (what, got["batches"], got["rows"])
    np.testing.assert_array_equal(got["correct"], ref.correct, err_msg=str(what))
    np.testing.assert_array_equal(got["confusion"], ref.confusion, err_msg=str(what))
    return got


def soft_ce(out, label):
    """fp64 mean over rows of -sum_c y log_softmax(out); an index label is one-hot."""
    o = out.astype(np.float64)
    if label.ndim == 1:
        y = np.zeros_like(o)
        y[np.arange(o.shape[0]), label] = 1.0
    else:
        y = label.astype(np.float64)
    mx = o.max(1, keepdims=True)
    lsm = o - (mx + np.log(np.exp(o - mx).sum(1, keepdims=True)))
    return float(-(y * lsm).sum(1).mean())


def _batch(rng, N, C, form, lo=-4.0, hi=4.0):
    out = rng.uniform(lo, hi, (N, C)).astype(np.float32)
    if form == "soft":
        label = rng.random((N, C)).astype(np.float32)
        label /= label.sum(1, keepdims=True)
    else:
        label = rng.integers(0, C, N).astype(np.int64)
    return out, label


def _to(d, *arrays):
    return [torch.from_numpy(a).to(d) for a in arrays]


# ---- 1. counts --------------------------------------------------------------------------------------
GRID = [(C, ks) for C in (2, 11, 17, 64) for ks in ((1,), (1, 5)) if max(ks) <= C] + [(11, (1, 2, 3, 4, 5, 6, 7, 8))]


@pytest.mark.parametrize("form", ["soft", "index"])
@pytest.mark.parametrize("C,top_k", GRID, ids=lambda v: str(v).replace(" ", ""))
def test_update_counts_match_numpy(C, top_k, form):
    """N in {1, 63, 64, 65, 257, 300} (one thread, a wave and its neighbours, more than one pass of the
    256-thread workgroup) x C (17 and 64 take the rows-in-memory path, 2 and 11 the register path):
    three updates with different batches into one block; every integer equals the reference."""
    from fall_multimodal_amd.metrics import StepMetrics
    d = dev()
    for N in (1, 63, 64, 65, 257, 300):
        rng = np.random.default_rng(1000 * C + 10 * N + len(top_k))
        m = StepMetrics(C, top_k, device=d)
        ref = Ref(C, top_k)
        for _ in range(3):
            out, label = _batch(rng, N, C, form)
            m.update(*_to(d, out, label))
            ref.add(out, label)
        assert_counts(m, ref, (N, C, top_k, form))
        m.reset()
        got = read_block(m)
        assert got["batches"] == 0 and got["rows"] == 0 and not got["confusion"].any() and got["loss_sum"] == 0.0


@pytest.mark.parametrize("C", [11, 17])
def test_update_ties_follow_the_lowest_index_rule(C):
    """Exact ties in the logits and in the soft label (three-valued entries): checked against the
    stated rule in numpy, not against torch."""
    from fall_multimodal_amd.metrics import StepMetrics
    d = dev()
    rng = np.random.default_rng(7 + C)
    top_k = (1, 2, 3, 5)
    out = rng.integers(0, 3, (300, C)).astype(np.float32)
    label = (rng.integers(0, 3, (300, C)) / 4).astype(np.float32)
    out[0], label[0] = 1.0, 0.25      # everything tied: class 0 is both the label and the prediction
    out[1], label[1, C - 1] = 2.0, 1.0  # all logits tied, last class true: rank C - 1
    m = StepMetrics(C, top_k, device=d)
    ref = Ref(C, top_k)
    m.update(*_to(d, out, label))
    ref.add(out, label)
    got = assert_counts(m, ref, C)
    assert got["confusion"][0, 0] >= 1 and got["confusion"][C - 1, 0] >= 1
    # and with index labels on the same tied logits
    idx = rng.integers(0, C, 300).astype(np.int64)
    m.update(*_to(d, out, idx))
    ref.add(out, idx)
    assert_counts(m, ref, C)


@pytest.mark.parametrize("C", [11, 17])
def test_update_nan_logit_orders_above_every_number(C):
    from fall_multimodal_amd.metrics import StepMetrics
    d = dev()
    rng = np.random.default_rng(11 + C)
    top_k = (1, 2)
    out, _ = _batch(rng, 8, C, "index")
    idx = np.array([3, 2, 4, 1, 0, 5, 6, 7], dtype=np.int64)
    out[0, 3] = np.nan            # the target itself: rank 0, predicted
    out[1, 5] = np.nan            # another class: it is the prediction, the target's rank is >= 1
    out[2, 1] = out[2, 4] = np.nan  # two NaN tie: the lower index first, target 4 has rank 1
    out[3, 1] = out[3, 4] = np.nan  # target 1 has rank 0
    m = StepMetrics(C, top_k, device=d)
    ref = Ref(C, top_k)
    m.update(*_to(d, out, idx))
    ref.add(out, idx)
    got = assert_counts(m, ref, C)
    rank, pred = ref_counts(out, idx, top_k)
    assert list(rank[:4]) == [0, rank[1], 1, 0] and rank[1] >= 1 and list(pred[:4]) == [3, 5, 1, 1]
    assert got["confusion"][3, 3] >= 1 and got["confusion"][2, 5] >= 1 and got["confusion"][4, 1] >= 1


# ---- 2. loss ------------------------------------------------------------------------------------------
def test_given_loss_is_summed_in_fp64_bit_for_bit():
    from fall_multimodal_amd.metrics import StepMetrics
    d = dev()
    rng = np.random.default_rng(3)
    m = StepMetrics(11, (1,), device=d)
    vals = np.array([0.1, 2.3456789, 1e-3, 7.25], dtype=np.float32)
    want = np.float64(0.0)
    for v in vals:
        out, label = _batch(rng, 9, 11, "soft")
        m.update(*_to(d, out, label), torch.from_numpy(np.array([v])).to(d))
        want = want + np.float64(v)
    got = read_block(m)
    assert got["batches"] == 4
    assert np.float64(got["loss_sum"]).tobytes() == np.float64(want).tobytes()
    assert float(m.loss_sum.item()) == float(want)  # the device view a data-parallel caller would all-reduce
    assert int(m.counts[0].item()) == 4 and int(m.counts[1].item()) == 36


@pytest.mark.parametrize("form", ["soft", "index"])
@pytest.mark.parametrize("C", [2, 11, 17, 64])
def test_computed_loss_matches_fp64_soft_ce(C, form):
    """loss=None: the kernel's own soft-target CE. |logit| <= 10, so |lse| <= 10 + ln 64 < 14.2; fp32
    expf / logf / the subtraction err by a few ulp of that (~4e-6 per row), and a mean of rows cannot
    exceed the per-row bound."""
    from fall_multimodal_amd.metrics import StepMetrics
    d = dev()
    rng = np.random.default_rng(40 + C)
    runs = []
    for _ in range(2):
        rng = np.random.default_rng(40 + C)
        m = StepMetrics(C, (1,), device=d)
        want = 0.0
        for N in (300, 65, 1):
            out, label = _batch(rng, N, C, form, -10.0, 10.0)
            m.update(*_to(d, out, label))
            want += soft_ce(out, label)
        got = read_block(m)
        print(f"C={C} {form}: loss_sum {got['loss_sum']!r} fp64 reference {want!r} diff {got['loss_sum'] - want:.3e}")
        np.testing.assert_allclose(got["loss_sum"], want, **LOSS_TOL)
        runs.append(m.block.clone())
    assert torch.equal(runs[0], runs[1])  # same inputs, same bits


# ---- 3. segment norms -----------------------------------------------------------------------------------
def test_segment_norms_match_fp64_and_never_read_padding():
    from fall_multimodal_amd.metrics import SegmentNorms
    d = dev()
    lens = [1, 3, 4, 5, 0, 1023, 4096, 4097, 600_001]
    offs, at = [], 4
    for n in lens:
        offs.append(at)
        at = (at + n + 3) // 4 * 4 + 4  # 16-byte aligned starts, at least four floats of padding between
    rng = np.random.default_rng(9)
    buf = np.full(at + 4, np.nan, dtype=np.float32)
    for k, (o, n) in enumerate(zip(offs, lens)):
        buf[o:o + n] = (rng.standard_normal(n) * 10.0 ** (k - 1)).astype(np.float32)
    flat = torch.from_numpy(buf).to(d)
    seg = SegmentNorms(flat, offs, lens)
    sq = [float((buf[o:o + n].astype(np.float64) ** 2).sum()) for o, n in zip(offs, lens)]
    want = np.sqrt(np.array(sq + [sum(sq)]))
    first = seg(1.0).clone()
    got = first.cpu().numpy().astype(np.float64)
    assert got.shape == (len(lens) + 1,)
    assert np.isfinite(got).all(), got  # a NaN would be padding read
    for s, (g, w) in enumerate(zip(got, want)):
        print(f"segment {s}: got {g!r} want {w!r} rel {abs(g - w) / w if w else 0.0:.2e}")
        assert abs(g - w) <= NORM_RTOL * w, (s, g, w)
    assert got[4] == 0.0  # the empty segment
    half = seg(0.5).clone().cpu().numpy().astype(np.float64)
    for s, (g, w) in enumerate(zip(half, 0.5 * want)):
        assert abs(g - w) <= NORM_RTOL * w, (s, g, w)
    assert torch.equal(seg(1.0), first)  # same bits on a second run
    assert torch.isnan(flat).sum().item() == int(np.isnan(buf).sum())  # the buffer is only read


def test_segment_norms_of_no_segments():
    from fall_multimodal_amd.metrics import SegmentNorms
    d = dev()
    seg = SegmentNorms(torch.ones(8, device=d), [], [])
    assert seg(1.0).cpu().tolist() == [0.0]


# ---- 4. TrainStep ----------------------------------------------------------------------------------------
B = 8


def _net(d, st):
    import fall_multimodal_amd as f3
    model = f3.TwoStreamSTGCAN_BiLSTM(3, {"layout": "coco_mmpose", "strategy": "spatial"}, 11, 6, device=d,
                                      precision="bf16x3")
    model.load_state_dict(st)
    return model


def _check_grad_norms(step, model):
    names, norms = step.param_grad_norms()
    assert names == [n for n, _ in model.named_parameters()]
    assert norms.dtype == torch.float32 and norms.is_cuda and norms.shape == (len(names) + 1,)
    got = norms.cpu().numpy().astype(np.float64)
    total = 0.0
    for (n, p), g in zip(model.named_parameters(), got):
        w = float(p.grad.double().norm().item())
        total += float((p.grad.double() ** 2).sum().item())
        assert abs(g - w) <= NORM_RTOL * w, (n, g, w)
    assert total > 0 and abs(got[-1] - np.sqrt(total)) <= NORM_RTOL * np.sqrt(total)
    return got


@pytest.mark.parametrize("mode", ["eager", "captured"])
def test_train_step_accumulates_and_only_reads(mode):
    """(a) three steps on three batches: the counters equal the host reference built from step.out and
    the label read after each step, loss_sum the fp64 sum of the three step.loss values; (b) capture()
    leaves the accumulators untouched; (c) the parameters equal, bit for bit, those of a twin step
    without metrics; param_grad_norms() after the last step (eager or replayed) matches p.grad."""
    import fall_multimodal_amd as f3
    d = dev()
    spec = oc.Spec(model="two_stgcan_bilstm", layout="coco_mmpose", num_class=11, sensor_dim=6)
    st = oc.init_state(spec, 61)
    batches = [[torch.from_numpy(x).to(d) for x in synthetic_batch(B, 18, 11, 6, 70 + i)] for i in range(3)]
    model, twin = _net(d, st), _net(d, st)
    step = f3.TrainStep(model, B, lr=1e-3, metrics=True)
    tstep = f3.TrainStep(twin, B, lr=1e-3)
    assert tstep.metrics is None and step.metrics.top_k == (1,)
    if mode == "captured":
        for s in (step, tstep):
            s.capture(*(t.clone() for t in batches[0]))
        blk = read_block(step.metrics)
        assert blk["batches"] == 0 and blk["rows"] == 0 and blk["loss_sum"] == 0.0       # (b)
        assert not blk["correct"].any() and not blk["confusion"].any()
    ref = Ref(11, (1,))
    loss_sum = np.float64(0.0)
    for sk, se, lb in batches:
        step(sk, se, lb)
        tstep(sk, se, lb)
        torch.cuda.synchronize()
        ref.add(step.out.cpu().numpy(), lb.cpu().numpy())
        loss_sum = loss_sum + np.float64(step.loss.cpu().numpy()[0])
    got = assert_counts(step.metrics, ref, mode)                                         # (a)
    assert np.float64(got["loss_sum"]).tobytes() == loss_sum.tobytes()
    res = step.metrics.result()
    assert res["batches"] == 3 and res["rows"] == 3 * B and res["loss"] == float(loss_sum) / 3
    assert res["top_k"] == [int(ref.correct[0]) / (3 * B)]
    assert torch.equal(model.flat_parameters(), twin.flat_parameters())                  # (c)
    assert torch.equal(model._flat_buffers, twin._flat_buffers)
    _check_grad_norms(step, model)


def test_train_step_rejects_foreign_metrics():
    import fall_multimodal_amd as f3
    d = dev()
    spec = oc.Spec(model="two_stgcan_bilstm", layout="coco_mmpose", num_class=11, sensor_dim=6)
    model = _net(d, oc.init_state(spec, 61))
    with pytest.raises(ValueError, match="StepMetrics"):
        f3.TrainStep(model, B, metrics=f3.StepMetrics(5, (1,), device=d))


def test_param_grad_norms_match_the_clipping_norm():
    """(d) with optimizer=SGD and max_norm set, the step's own grad_norm is populated: the global entry
    matches it, and every per-tensor entry matches p.grad."""
    import fall_multimodal_amd as f3
    d = dev()
    spec = oc.Spec(model="two_stgcan_bilstm", layout="coco_mmpose", num_class=11, sensor_dim=6)
    model = _net(d, oc.init_state(spec, 61))
    step = f3.TrainStep(model, B, optimizer=f3.SGD(model.parameters(), lr=1e-3), max_norm=10)
    sk, se, lb = (torch.from_numpy(x).to(d) for x in synthetic_batch(B, 18, 11, 6, 70))
    step(sk, se, lb)
    got = _check_grad_norms(step, model)
    ref = float(step.grad_norm.item())
    assert ref > 0 and abs(got[-1] - ref) <= NORM_RTOL * ref, (got[-1], ref)


# ---- 5. valid_device / test_device ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eval_setup():
    """80 synthetic windows behind a batch-32 loader (last batch 16), a model with non-trivial running
    statistics; the device-side results and the per-batch logits they were computed from."""
    import fall_multimodal_amd as f3
    from fall_multimodal_amd import data as fd
    from fall_multimodal_amd import evaluate as fe
    d = dev()
    spec = oc.Spec(model="two_stgcan_bilstm", layout="coco_mmpose", num_class=11, sensor_dim=6)
    model = f3.TwoStreamSTGCAN_BiLSTM(3, {"layout": "coco_mmpose", "strategy": "spatial"}, 11, 6, device=d)
    model.load_state_dict(oc.init_state(spec, 31))
    model.train()
    with torch.no_grad():  # one train-mode forward moves the BN running statistics
        model(*(torch.from_numpy(x).to(d) for x in synthetic_batch(64, 18, 11, 6, 20)[:2]))
    skel, sensor, label = synthetic_batch(80, 18, 11, 6, 21)
    w = fd.Windows([f"v{i // 4}" for i in range(80)], np.ascontiguousarray(skel.transpose(0, 2, 3, 1)), sensor, label)
    loader = fd.WindowLoader(w, 32, shuffle=False, drop_last=False, device=d)
    assert model.training
    res_t = fe.test_device(model, loader, top_k=(1, 5))
    res_v = fe.valid_device(model, loader, top_k=(1, 5))
    assert model.training  # the mode is restored
    out, lab = fe.predict(model, loader)
    return {"model": model, "loader": loader, "test": res_t, "valid": res_v,
            "out": out.cpu().numpy(), "label": lab.cpu().numpy()}


def test_eval_device_matches_numpy(eval_setup):
    s = eval_setup
    out, label, res = s["out"], s["label"], s["test"]
    assert out.shape == (80, 11)
    ref = Ref(11, (1, 5))
    losses = []
    for lo, hi in ((0, 32), (32, 64), (64, 80)):  # the loader's batches, the last one smaller
        ref.add(out[lo:hi], label[lo:hi])
        losses.append(soft_ce(out[lo:hi], label[lo:hi]))
    assert res["confusion"] == ref.confusion.tolist()
    assert res["top_k"] == [int(ref.correct[0]) / 80, int(ref.correct[1]) / 80]
    print(f"device loss {res['loss']!r} fp64 reference {float(np.mean(losses))!r}")
    np.testing.assert_allclose(res["loss"], float(np.mean(losses)), **LOSS_TOL)
    assert set(res) == {"loss", "top_k", "precision", "recall", "f1", "specificity", "confusion"}
    assert s["valid"] == {"loss": res["loss"], "top_k": res["top_k"]}


def test_eval_device_matches_evaluate_test(eval_setup):
    pytest.importorskip("sklearn")
    from fall_multimodal_amd import evaluate as fe
    s = eval_setup
    want = fe.test(s["model"], s["loader"], torch.nn.CrossEntropyLoss(), top_k=(1, 5), num_classes=11)
    got = s["test"]
    assert got["top_k"] == want["top_k"] and got["confusion"] == want["confusion"]
    for k in ("precision", "recall", "f1"):
        assert abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k])
    np.testing.assert_allclose(got["specificity"], want["specificity"], rtol=0, atol=1e-12)
    print(f"device loss {got['loss']!r} evaluate.test loss {want['loss']!r}")
    np.testing.assert_allclose(got["loss"], want["loss"], **LOSS_TOL)
    wv = fe.valid(s["model"], s["loader"], torch.nn.CrossEntropyLoss(), top_k=(1, 5))
    assert s["valid"]["top_k"] == wv["top_k"]
    np.testing.assert_allclose(s["valid"]["loss"], wv["loss"], **LOSS_TOL)
