"""The flat-storage base and the fused steps on the device: a model built on the CPU and moved with
.to("cuda") keeps its values and its aliasing, and one fused step (TrainStep at B=2, the side steps
at B=4) leaves a finite loss, a non-zero flat gradient and .grad views into it. No numbers are compared
here: the parity tests of each model cover the kernels."""
import pytest
import torch

from tests.test_flat_module import COUNTERS, MODELS, check_order_and_aliasing

pytestmark = pytest.mark.gpu


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda")


def _fall3_step(model, d):
    import fall_multimodal_amd as f3
    from oracle.prng import synthetic_batch
    skel, sensor, label = synthetic_batch(2, model.num_node, 11, model.spec.sensor_dim, 3)
    step = f3.TrainStep(model, 2, lr=1e-3)
    return step, [torch.from_numpy(a).to(d) for a in (skel, sensor, label)]


def _targcn_step(model, d):
    import fall_multimodal_amd as f3
    from oracle import targcn_cpu as tg
    source, label = tg.synthetic_source(4, model.num_node, 11, 3)
    return f3.TargcnStep(model, 4), [torch.from_numpy(a).to(d) for a in (source, label)]


def _sktr_step(model, d):
    import fall_multimodal_amd as f3
    from oracle import sktr_cpu as sk
    x, label = sk.synthetic_clips(4, 14, 11, 3)
    return f3.SktrStep(model, 4), [torch.from_numpy(a).to(d) for a in (x, label)]


def _musa_step(model, d):
    from fall_multimodal_amd import musa
    from oracle.prng import synthetic_batch
    x, _, label = synthetic_batch(4, 14, 11, 1, 3)
    return musa.MusaStep(model, 4), [torch.from_numpy(a).to(d) for a in (x, label)]


STEPS = {"fall3": _fall3_step, "fall3_notebook": _fall3_step, "targcn": _targcn_step, "sktr": _sktr_step,
         "musa": _musa_step}


@pytest.mark.parametrize("kind", list(MODELS))
def test_move_to_device_then_one_fused_step(kind):
    d = dev()
    torch.manual_seed(11)
    model = MODELS[kind]()
    cpu_values = {k: v.clone() for k, v in model.state_dict().items()}
    params = list(model.parameters())
    assert model.to(d) is model
    assert all(a is b for a, b in zip(model.parameters(), params))
    assert model.flat_parameters().is_cuda and model._flat_buffers.is_cuda
    check_order_and_aliasing(model, COUNTERS[kind])
    sd = model.state_dict()
    assert list(sd.keys()) == list(cpu_values.keys())
    for k, v in cpu_values.items():
        got = sd[k].cpu()
        assert got.dtype == v.dtype and got.numpy().tobytes() == v.numpy().tobytes(), k

    step, batch = STEPS[kind](model, d)
    model.train()
    loss = step(*batch)
    torch.cuda.synchronize()
    assert loss is step.loss and bool(torch.isfinite(step.loss).all())
    assert step.grads.numel() == model._native.nparam and bool(torch.isfinite(step.grads).all())
    assert int(torch.count_nonzero(step.grads)) > 0
    if kind == "musa":
        from fall_multimodal_amd.musa import grad_is_none
        none = lambda name: grad_is_none(name, model.dropblock)  # noqa: E731
    else:
        none = lambda name: False  # noqa: E731
    for (name, p), (_, shape, off) in zip(model.named_parameters(), model.param_views()):
        if none(name):
            assert p.grad is None, name
        else:
            assert p.grad is not None and tuple(p.grad.shape) == tuple(shape) and p.grad.is_contiguous(), name
            assert p.grad.data_ptr() == step.grads.data_ptr() + 4 * off, name
    if kind == "musa":
        assert any(p.grad is None for p in model.parameters())
    if len(batch) == 2:  # the side steps refuse a label that is not on the input's device, before any launch
        with pytest.raises(ValueError, match=type(step).__name__):
            step(batch[0], batch[1].cpu())
