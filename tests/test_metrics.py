"""Device-side step metrics, the parts that need no GPU: the C ABI declares and exports the five
functions, their host-side argument checks reject bad calls before any launch, and
metrics.summarize (pure numpy) reproduces a direct fp64 restatement of the macro metrics and,
where sklearn is installed, evaluate.class_metrics on labels with the same confusion matrix."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("f3_metrics_bytes", "f3_metrics_reset", "f3_metrics_update", "f3_segment_norms_scratch_bytes",
         "f3_segment_norms")


def test_header_declares_and_library_exports_the_metrics_functions():
    import fall_multimodal_amd._lib as L
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fall3.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(f3_\w+)\s*\(", src))
    so = L.lib()
    for f in FUNCS:
        assert f in declared, f
        assert f in L.EXPORTS, f
        assert getattr(so, f).argtypes is not None, f
    assert "#define F3_METRICS_MAXK 8" in src and L.METRICS_MAXK == 8


def test_block_and_scratch_sizes():
    import fall_multimodal_amd._lib as L
    so = L.lib()
    # fp64 loss_sum, int64 batches, rows, correct[8], confusion[C*C]
    for C in (1, 2, 11, 64):
        assert so.f3_metrics_bytes(C) == 8 * (3 + 8 + C * C)
    assert so.f3_metrics_bytes(0) == 0 and so.f3_metrics_bytes(65) == 0
    # room for every segment's rounded-up chunk count, and never empty
    assert so.f3_segment_norms_scratch_bytes(0, 0) >= 8
    for total, nseg in ((1, 1), (8192, 1), (8193, 2), (10 ** 6, 300)):
        assert so.f3_segment_norms_scratch_bytes(total, nseg) >= 8 * (total // 8192 + nseg)


def test_update_rejects_bad_arguments_before_any_launch():
    """F3_EINVAL comes from the host-side checks, so fake (never dereferenced) pointers do."""
    import fall_multimodal_amd._lib as L
    so = L.lib()
    P = ctypes.c_void_p
    acc, out, lab, idx = P(0x1000), P(0x2000), P(0x3000), P(0x4000)

    def upd(label, label_idx, C, ks, N=4):
        k = (ctypes.c_int * max(len(ks), 1))(*ks)
        return so.f3_metrics_update(acc, out, label, label_idx, None, N, C, k, len(ks), None)

    assert upd(lab, idx, 11, (1,)) == L.F3_EINVAL        # both label forms
    assert upd(None, None, 11, (1,)) == L.F3_EINVAL      # neither
    assert upd(lab, None, 0, ()) == L.F3_EINVAL          # C < 1
    assert upd(lab, None, 65, (1,)) == L.F3_EINVAL       # C > 64
    assert upd(lab, None, 11, (1, 12)) == L.F3_EINVAL    # k > C
    assert upd(lab, None, 11, (0,)) == L.F3_EINVAL       # k < 1
    assert upd(lab, None, 11, tuple(range(1, 10))) == L.F3_EINVAL  # nk > F3_METRICS_MAXK
    assert upd(lab, None, 11, (1,), N=0) == L.F3_EINVAL
    assert so.f3_metrics_reset(acc, 65, None) == L.F3_EINVAL
    assert so.f3_metrics_reset(None, 11, None) == L.F3_EINVAL
    assert so.f3_segment_norms(out, lab, idx, -1, acc, acc, 8, 1.0, None) == L.F3_EINVAL
    assert so.f3_segment_norms(out, lab, idx, 1, acc, acc, 0, 1.0, None) == L.F3_EINVAL   # no scratch
    assert so.f3_segment_norms(P(0x2004), lab, idx, 1, acc, acc, 8, 1.0, None) == L.F3_EINVAL  # g not 16-B aligned


def test_step_metrics_argument_validation():
    import fall_multimodal_amd as f3
    from fall_multimodal_amd import metrics as fm
    assert f3.StepMetrics is fm.StepMetrics and f3.summarize is fm.summarize
    with pytest.raises(ValueError, match="top_k"):
        fm.StepMetrics(5, top_k=(1, 6))
    with pytest.raises(ValueError, match="top_k"):
        fm.StepMetrics(11, top_k=(0,))
    with pytest.raises(ValueError, match="num_class"):
        fm.StepMetrics(65)
    with pytest.raises(ValueError, match="at most 8"):
        fm.StepMetrics(11, top_k=tuple(range(1, 10)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        fm.StepMetrics(11, device="cpu")
    # update()'s checks: a CPU tensor is refused (there is no CPU path), before shapes are looked at
    out, lab = torch.zeros(4, 11), torch.zeros(4, 11)
    with pytest.raises(RuntimeError, match="HIP device"):
        fm.check_batch(out, lab, None, 11)
    with pytest.raises(RuntimeError, match="HIP device"):
        fm.check_batch(out, torch.zeros(4, dtype=torch.int64), None, 11)


def _direct(cm):
    """The macro metrics restated class by class in fp64 (python floats)."""
    cm = np.asarray(cm, dtype=np.int64)
    C, total = cm.shape[0], int(cm.sum())
    P, R, F, S = [], [], [], []
    for c in range(C):
        tp = int(cm[c, c])
        true_c, pred_c = int(cm[c, :].sum()), int(cm[:, c].sum())
        fp, fn = pred_c - tp, true_c - tp
        tn = total - tp - fp - fn
        S.append(tn / (tn + fp) if tn + fp > 0 else 0.0)
        if true_c + pred_c == 0:
            continue  # the class occurs nowhere: not part of the macro average
        P.append(tp / pred_c if pred_c else 0.0)
        R.append(tp / true_c if true_c else 0.0)
        F.append(2 * tp / (true_c + pred_c))
    return float(np.mean(P)), float(np.mean(R)), float(np.mean(F)), S


def _cases():
    rng = np.random.default_rng(5)
    dense = rng.integers(0, 40, (11, 11))
    absent = rng.integers(0, 40, (11, 11))
    absent[4, :] = 0
    absent[:, 4] = 0          # class 4 occurs neither as a label nor as a prediction
    never = rng.integers(1, 40, (7, 7))
    never[:, 2] = 0           # class 2 is never predicted (precision 0/0 -> 0), but occurs as a label
    unseen = rng.integers(1, 40, (7, 7))
    unseen[5, :] = 0          # class 5 is predicted but never true (recall 0/0 -> 0)
    two = rng.integers(0, 40, (2, 2))
    return {"dense": dense, "absent_class": absent, "never_predicted": never, "never_true": unseen, "C2": two}


def _ulp_close(a, b):
    return a == b or abs(a - b) <= np.spacing(max(abs(a), abs(b)))


@pytest.mark.parametrize("name", list(_cases()))
def test_summarize_matches_direct_restatement(name):
    from fall_multimodal_amd.metrics import summarize
    cm = _cases()[name]
    rows = int(cm.sum())
    got = summarize(3.75, 3, rows, [int(np.trace(cm)), rows, 0, 0, 0, 0, 0, 0], cm, (1, 2))
    p, r, f, s = _direct(cm)
    assert _ulp_close(got["precision"], p) and _ulp_close(got["recall"], r) and _ulp_close(got["f1"], f)
    assert got["specificity"] == s
    assert got["confusion"] == cm.tolist()
    assert got["loss"] == 1.25 and got["batches"] == 3 and got["rows"] == rows
    assert got["top_k"] == [int(np.trace(cm)) / rows, 1.0]


def test_summarize_empty_block():
    from fall_multimodal_amd.metrics import summarize
    got = summarize(0.0, 0, 0, [0] * 8, np.zeros((3, 3), dtype=np.int64), (1,))
    assert got["loss"] is None and got["top_k"] == [None] and got["rows"] == 0
    assert (got["precision"], got["recall"], got["f1"]) == (0.0, 0.0, 0.0)
    assert got["specificity"] == [0.0, 0.0, 0.0]


@pytest.mark.parametrize("name", list(_cases()))
def test_summarize_matches_class_metrics(name):
    pytest.importorskip("sklearn")
    from fall_multimodal_amd.evaluate import class_metrics
    from fall_multimodal_amd.metrics import summarize
    cm = _cases()[name]
    C = cm.shape[0]
    true = np.concatenate([np.full(int(cm[t, p]), t) for t in range(C) for p in range(C)])
    pred = np.concatenate([np.full(int(cm[t, p]), p) for t in range(C) for p in range(C)])
    ref = class_metrics(pred, true, C)
    got = summarize(0.0, 1, int(cm.sum()), [0] * 8, cm, (1,))
    assert got["confusion"] == ref["confusion"]
    for k in ("precision", "recall", "f1"):
        assert _ulp_close(got[k], ref[k]), (k, got[k], ref[k])
    assert len(got["specificity"]) == C
    for a, b in zip(got["specificity"], ref["specificity"]):
        assert _ulp_close(a, b)
