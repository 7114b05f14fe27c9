"""Class-weighted cross-entropy without a GPU: TrainStep's check of the weights, data.class_weights against
sklearn, and an fp32 numpy emulation of f3_soft_ce_w's sums (W in fp64) inside the two gates of
tests/class_weight_ref.py for exactly the cases tests/test_gpu_class_weight.py runs on the device: the
gates are reachable before a GPU is involved."""
import numpy as np
import pytest
import torch

from tests import class_weight_ref as R


# ---- check_class_weight ----------------------------------------------------------------------------
def test_check_class_weight_accepts_list_ndarray_tensor():
    from fall_multimodal_amd.train import check_class_weight
    want = np.array([1.0, 0.5, 0.0, 4.0], dtype=np.float32)
    for w in ([1.0, 0.5, 0.0, 4.0], (1, 0.5, 0, 4), np.array([1.0, 0.5, 0.0, 4.0]),
              np.array([1.0, 0.5, 0.0, 4.0], dtype=np.float32), torch.tensor([1.0, 0.5, 0.0, 4.0]),
              torch.tensor([1.0, 0.5, 0.0, 4.0], dtype=torch.float64)):
        got = check_class_weight(w, 4)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (4,)
        np.testing.assert_array_equal(got, want)
    ints = check_class_weight(np.array([1, 2, 3]), 3)
    assert ints.dtype == np.float32 and ints.tolist() == [1.0, 2.0, 3.0]
    held = np.array([1.0, 2.0])
    check_class_weight(held, 2)[0] = 9.0  # the result is the caller's own array
    assert held.tolist() == [1.0, 2.0]


@pytest.mark.parametrize("bad", [
    [1.0, 2.0, 3.0],                      # wrong length
    [1.0, 2.0, 3.0, 4.0, 5.0],
    [[1.0, 2.0], [3.0, 4.0]],             # 2-D
    np.ones((1, 4)),
    [1.0, -0.5, 1.0, 1.0],                # a negative
    [1.0, float("nan"), 1.0, 1.0],
    [1.0, float("inf"), 1.0, 1.0],
    [0.0, 0.0, 0.0, 0.0],                 # all zeros
    [True, False, True, True],            # bools
    np.array([True, True, True, True]),
    "1234",                               # a string
    ["1", "2", "3", "4"],
    [1.0, 1e300, 1.0, 1.0],               # finite, but not in float32
    None,
    4.0,
], ids=lambda b: repr(b)[:24])
def test_check_class_weight_refuses(bad):
    from fall_multimodal_amd.train import check_class_weight
    with pytest.raises(ValueError):
        check_class_weight(bad, 4)


# ---- data.class_weights ------------------------------------------------------------------------------
def test_class_weights_are_sklearns_balanced():
    from sklearn.utils.class_weight import compute_class_weight
    from fall_multimodal_amd import data as fd
    rng = np.random.default_rng(3)
    C = 11
    idx = np.concatenate([np.arange(C), rng.choice(C, 500, p=np.linspace(1, 12, C) / np.linspace(1, 12, C).sum())])
    want = compute_class_weight("balanced", classes=np.arange(C), y=idx)
    got = fd.class_weights(idx)
    assert got.dtype == np.float32 and got.shape == (C,)
    np.testing.assert_array_equal(got, want.astype(np.float32))
    onehot = np.eye(C, dtype=np.float32)[idx]
    np.testing.assert_array_equal(fd.class_weights(onehot), got)
    soft = onehot * 0.9 + 0.1 / C  # argmax keeps the class
    np.testing.assert_array_equal(fd.class_weights(torch.from_numpy(soft)), got)
    np.testing.assert_array_equal(fd.class_weights(torch.from_numpy(idx), num_class=C), got)


def test_class_weights_absent_class_and_refusals():
    from fall_multimodal_amd import data as fd
    from fall_multimodal_amd.train import check_class_weight
    idx = np.array([0, 0, 0, 2, 2, 4])
    w = fd.class_weights(idx, num_class=6)
    assert w.tolist() == [np.float32(6 / (6 * 3)), 0.0, np.float32(6 / (6 * 2)), 0.0, 1.0, 0.0]
    check_class_weight(w, 6)  # what the helper gives, the step accepts
    assert fd.class_weights(idx).shape == (5,)
    assert fd.class_weights(np.eye(6, dtype=np.float32)[idx]).tolist() == w.tolist()
    with pytest.raises(ValueError):
        fd.class_weights(idx, scheme="sqrt")
    with pytest.raises(ValueError):
        fd.class_weights(idx, num_class=3)
    with pytest.raises(ValueError):
        fd.class_weights(np.eye(6)[idx], num_class=5)
    with pytest.raises(ValueError):
        fd.class_weights(np.zeros((2, 3, 4)))
    with pytest.raises(ValueError):
        fd.class_weights(np.array([], dtype=np.int64))


# ---- the ABI ----------------------------------------------------------------------------------------
def test_weighted_loss_is_declared_and_bound():
    import fall_multimodal_amd._lib as L
    assert "f3_soft_ce_w" in L.EXPORTS and "f3_net_loss_w" in L.EXPORTS
    lib = L.lib()
    assert len(lib.f3_soft_ce_w.argtypes) == 10 and len(lib.f3_net_loss_w.argtypes) == 9


# ---- the rules written out are torch's ---------------------------------------------------------------
@pytest.mark.parametrize("form", R.FORMS)
def test_written_out_rules_match_torch_in_fp64(form):
    """loss = -(1/D) sum a lsm and dout = (softmax m - a) / D with the a, m and D of class_weight_ref.scales."""
    for C in (1, 2, 11, 17):
        for N in (1, 5, 64):
            for eps in R.SMOOTHINGS:
                out, label, w = R.make_case(N, C, form, eps)
                want_l, want_d = R.torch_reference(out, label, w, eps)
                o = out.astype(np.float64)
                lsm = o - (o.max(1, keepdims=True) + np.log(np.exp(o - o.max(1, keepdims=True)).sum(1, keepdims=True)))
                w64 = w.astype(np.float64)
                if label.ndim == 1:
                    live = R.live_rows(label, C)
                    y = np.zeros((N, C))
                    y[np.flatnonzero(live), label[live]] = 1.0
                    a = (y * (1 - eps) + eps / C) * w64 * live[:, None]
                else:
                    a = (label.astype(np.float64) * (1 - eps) + eps / C) * w64
                m, D = R.scales(label, w, eps, C)
                np.testing.assert_allclose(m, a.sum(1), rtol=1e-15)
                np.testing.assert_allclose(-(a * lsm).sum() / D, want_l, rtol=1e-13, atol=1e-15)
                np.testing.assert_allclose((np.exp(lsm) * m[:, None] - a) / D, want_d, rtol=0, atol=1e-14)


# ---- the fp32 emulation inside the gates ---------------------------------------------------------------
@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("C", R.CLASSES)
def test_fp32_emulation_with_fp64_W_is_inside_the_gates(C, form):
    worst_l = worst_d = 0.0
    for N in R.BATCHES:
        for eps in R.SMOOTHINGS:
            out, label, w = R.make_case(N, C, form, eps)
            loss, dout = R.emulate(out, label, w, eps)
            assert np.isfinite(loss) and np.isfinite(dout).all(), (N, C, form, eps)
            rl, rd = R.gate_ratios(loss, dout, out, label, w, eps)
            worst_l, worst_d = max(worst_l, rl), max(worst_d, rd)
            assert rl <= 1.0 and rd <= 1.0, (N, C, form, eps, rl, rd)
            if label.ndim == 1:
                dead = ~R.live_rows(label, C)
                assert not dout[dead].any()
    print(f"C={C} {form}: emulation worst loss gate ratio {worst_l:.4f}, worst dout gate ratio {worst_d:.4f}")
