"""Label smoothing and gradient accumulation in the fused step, the parts that need no device: the
reference's update rule (model/main.py:115-132), the TRAIN.* plumbing and the argument checks."""
import numpy as np
import pytest


def test_accum_updates_is_the_reference_rule():
    """`i % accum_iter == 0 or i + 1 == len(dataloader)`, enumerated literally."""
    from fall_multimodal_amd.train import accum_updates
    for L in range(1, 13):
        for k in range(1, 6):
            want = []
            for i in range(L):
                want.append(bool(i % k == 0 or i + 1 == L))
            got = accum_updates(L, k)
            assert got == want, (L, k, got, want)
            assert all(type(v) is bool for v in got)
            assert got[0] and got[-1]  # batch 0 steps alone (the reference's quirk), and the epoch's last batch
    assert accum_updates(5, 3) == [True, False, False, True, True]
    assert accum_updates(7, 1) == [True] * 7
    assert accum_updates(0, 3) == []


def test_step_kwargs_reads_the_three_train_keys():
    from fall_multimodal_amd.config import get_cfg_defaults
    from fall_multimodal_amd.train import check_step_args, step_kwargs
    cfg = get_cfg_defaults()
    kw = step_kwargs(cfg)
    assert kw == {"max_norm": 100, "label_smoothing": 0.0, "accum_iter": 1}
    assert check_step_args(kw["label_smoothing"], kw["accum_iter"]) == (0.0, 1)
    cfg.merge_from_dict({"TRAIN": {"LABEL_SMOOTHING": 0.1, "ACCUM_ITER": 4, "MAX_NORM": 5.0}})
    assert step_kwargs(cfg) == {"max_norm": 5.0, "label_smoothing": 0.1, "accum_iter": 4}
    cfg.merge_from_list(["TRAIN.ACCUM_ITER", "2", "TRAIN.MAX_NORM", "None"])
    assert step_kwargs(cfg) == {"max_norm": None, "label_smoothing": 0.1, "accum_iter": 2}


@pytest.mark.parametrize("bad", [0, -1, 2.0, 2.5, "2", None, True])
def test_accum_iter_must_be_a_positive_integer(bad):
    from fall_multimodal_amd.train import accum_updates, check_step_args
    with pytest.raises(ValueError, match="accum_iter"):
        check_step_args(0.0, bad)
    with pytest.raises(ValueError, match="accum_iter"):
        accum_updates(4, bad)


@pytest.mark.parametrize("bad", [-0.1, 1.5, float("nan"), float("inf"), "0.1", None, True])
def test_label_smoothing_must_lie_in_the_unit_interval(bad):
    from fall_multimodal_amd.train import check_step_args
    with pytest.raises(ValueError, match="label_smoothing"):
        check_step_args(bad, 1)


def test_accepted_arguments_are_normalised():
    from fall_multimodal_amd.train import check_step_args
    assert check_step_args(0, 1) == (0.0, 1)
    assert check_step_args(1, np.int64(3)) == (1.0, 3)
    eps, k = check_step_args(np.float32(0.25), 2)
    assert eps == 0.25 and type(eps) is float and type(k) is int


def test_train_step_checks_before_it_builds_anything():
    """The constructor raises on the two settings before it touches the model (None here)."""
    import fall_multimodal_amd as f3
    with pytest.raises(ValueError, match="accum_iter"):
        f3.TrainStep(None, 8, accum_iter=0)
    with pytest.raises(ValueError, match="label_smoothing"):
        f3.TrainStep(None, 8, label_smoothing=1.5)
    with pytest.raises(ValueError, match="phased"):
        f3.TrainStep(None, 8, accum_iter=2, phased=True)
