"""skip_nonfinite, the device-side guard that skips an optimizer update on an inf / NaN gradient:
everything that needs no GPU. The header's declarations, the ctypes mirror of f3_optim_config, the
layout of the guard words in the step-scalar block, host-side refusals and TrainStep's argument check.
The kernels are held to the contract in tests/test_gpu_optim_guard.py."""
import ctypes
import inspect
import os
import re

import pytest
import torch

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fall3.h")

BASE = dict(kind=2, nesterov=False, lr=1e-3, alpha=0.99, eps=1e-8, momentum=0.0, beta1=0.9, beta2=0.999,
            weight_decay=0.0, max_norm=0.0, grad_scale=1.0)


def test_header_declares_the_field_and_the_entry():
    from fall_multimodal_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bf3_optim_guard_offset\s*\(", src)
    cfg = re.search(r"typedef struct f3_optim_config \{(.*?)\} f3_optim_config;", src, flags=re.S).group(1)
    fields = [re.split(r"[\s\[]", f.strip().split()[-1])[0] for f in cfg.split(";") if f.strip()]
    assert fields[-1] == "skip_nonfinite" and fields[-2] == "skip_len", fields  # the last field, after skip_len
    assert re.search(r"\bint\s+skip_nonfinite\s*;", cfg)
    assert "f3_optim_guard_offset" in _lib.EXPORTS
    assert hasattr(_lib.lib(), "f3_optim_guard_offset")


def test_config_mirror_and_block_layout():
    from fall_multimodal_amd import _lib, ops
    F = _lib.F3OptimConfig._fields_
    assert F[-1][0] == "skip_nonfinite" and F[-1][1] is ctypes.c_int
    assert tuple(n for n, t in F if t is ctypes.c_double) == ops.HYPER_FIELDS  # no double added
    L = _lib.lib()
    assert L.f3_optim_hyper_bytes() == 72  # the guard is structure, never a value in the hyper block
    off, size = int(L.f3_optim_guard_offset()), int(L.f3_optim_scalars_bytes())
    assert off % 8 == 0 and off + 16 <= size
    assert off >= 24  # behind t, the four fp32 scalars and the partials
    # the views ops hands out sit on those bytes
    block = torch.zeros(size // 4, dtype=torch.float32)
    skipped, last = ops.guard_views(block)
    assert skipped.dtype == torch.int64 and last.dtype == torch.int32 and skipped.numel() == last.numel() == 1
    skipped.fill_(3)
    last.fill_(1)
    raw = block.view(torch.int32)
    assert raw[off // 4:off // 4 + 3].tolist() == [3, 0, 1] and int(raw.count_nonzero()) == 2
    assert all(int(v.view(torch.int32).count_nonzero()) == 0 for v in ops.scalar_views(block))


def test_optim_config_defaults_the_field_to_zero():
    from fall_multimodal_amd import ops
    assert ops.optim_config(**BASE).skip_nonfinite == 0
    assert ops.optim_config(**BASE, skip=(0, 4)).skip_nonfinite == 0
    assert ops.optim_config(**BASE, skip_nonfinite=True).skip_nonfinite == 1
    assert ops.optim_config(*BASE.values()).skip_nonfinite == 0  # positional callers are unaffected
    assert list(inspect.signature(ops.optim_config).parameters)[-2:] == ["skip", "skip_nonfinite"]


def test_ranges_update_refuses_the_guard():
    """The decision needs every gradient: F3_EINVAL from f3_optim_step_ranges before anything touches the
    device (host-side validation, as for max_norm > 0), for every kind; the same call without the guard
    passes validation only on a device, so only the refusal is checked here."""
    from fall_multimodal_amd import _lib, ops
    L = _lib.lib()
    dummy = torch.zeros(64)  # host memory: never dereferenced, the calls fail validation first
    lo, ln = (ctypes.c_int64 * 1)(0), (ctypes.c_int64 * 1)(16)

    def status(**over):
        c = ops.optim_config(**{**BASE, **over})
        return L.f3_optim_step_ranges(c, _lib.ptr(dummy), _lib.ptr(dummy), _lib.ptr(dummy), _lib.ptr(dummy), 1, lo,
                                      ln, _lib.ptr(dummy), None)

    for kind in (_lib.OPT_RMSPROP, _lib.OPT_SGD, _lib.OPT_ADAM, _lib.OPT_ADAMW):
        assert status(kind=kind, skip_nonfinite=True) == _lib.F3_EINVAL
    assert status(max_norm=1.0) == _lib.F3_EINVAL  # the neighbouring refusal it is modelled on
    # a guarded plain-RMSprop step keeps a device count: the recorded form then needs the scalars too
    c = ops.optim_config(**{**BASE, "kind": _lib.OPT_RMSPROP}, skip_nonfinite=True)
    assert L.f3_optim_step_hyper(c, _lib.ptr(dummy), _lib.ptr(dummy), None, _lib.ptr(dummy), 16, _lib.ptr(dummy), None,
                                 None) == _lib.F3_EINVAL


@pytest.mark.parametrize("bad", [1, 0, None, "yes", 1.0])
def test_trainstep_takes_a_bool_only(bad):
    """Checked before anything else, so no model or device is needed to see it."""
    import fall_multimodal_amd as f3
    with pytest.raises(ValueError, match="skip_nonfinite"):
        f3.TrainStep(None, 4, skip_nonfinite=bad)


def test_trainstep_setting_is_off_by_default_and_read_only():
    import fall_multimodal_amd as f3
    sig = inspect.signature(f3.TrainStep.__init__)
    assert sig.parameters["skip_nonfinite"].default is False
    assert list(sig.parameters)[-1] == "skip_nonfinite"  # a trailing keyword: every existing call keeps working
    prop = f3.TrainStep.skip_nonfinite
    assert isinstance(prop, property) and prop.fset is None
    for name in ("skipped_steps", "steps_taken"):
        assert callable(getattr(f3.TrainStep, name))
