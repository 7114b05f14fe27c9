"""TrainStep(ema_decay=...), the parameter EMA kept on the device: everything that needs no GPU. The
header's declarations, the ctypes bindings, the layout of the 16-byte EMA block, the host-side refusals of
f3_ema_set_decay / f3_ema_update and TrainStep's argument check. The kernel and the step are held to the
contract in tests/test_gpu_ema.py."""
import ctypes
import inspect
import os
import re

import pytest
import torch

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fall3.h")
ENTRIES = ("f3_ema_state_bytes", "f3_ema_set_decay", "f3_ema_update")


def test_header_declares_the_three_entries():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint64_t\s+f3_ema_state_bytes\s*\(\s*void\s*\)\s*;", src)
    assert re.search(r"\bint\s+f3_ema_set_decay\s*\(\s*void\s*\*\s*state\s*,\s*double\s+decay\s*,\s*void\s*\*\s*stream\s*\)\s*;",
                     src)
    assert re.search(r"\bint\s+f3_ema_update\s*\(\s*float\s*\*\s*ema\s*,\s*const\s+float\s*\*\s*params\s*,\s*int64_t\s+n\s*,"
                     r"\s*void\s*\*\s*state\s*,\s*void\s*\*\s*stream\s*\)\s*;", src)


def test_exports_and_signatures():
    from fall_multimodal_amd import _lib
    L = _lib.lib()
    for name in ENTRIES:
        assert name in _lib.EXPORTS
        assert hasattr(L, name)
    P, I64 = ctypes.c_void_p, ctypes.c_int64
    assert L.f3_ema_state_bytes.restype is I64 and list(L.f3_ema_state_bytes.argtypes) == []
    assert L.f3_ema_set_decay.restype is ctypes.c_int
    assert list(L.f3_ema_set_decay.argtypes) == [P, ctypes.c_double, P]
    assert L.f3_ema_update.restype is ctypes.c_int and list(L.f3_ema_update.argtypes) == [P, P, I64, P, P]


def test_block_is_16_bytes_and_the_views_sit_on_bytes_0_and_8():
    from fall_multimodal_amd import _lib, ops
    assert int(_lib.lib().f3_ema_state_bytes()) == 16
    block = ops.ema_state("cpu")
    assert block.numel() * block.element_size() == 16 and int(block.view(torch.int32).count_nonzero()) == 0
    count, decay = ops.ema_views(block)
    assert count.dtype == torch.int64 and decay.dtype == torch.float64 and count.numel() == decay.numel() == 1
    assert count.data_ptr() == block.data_ptr() and decay.data_ptr() == block.data_ptr() + 8
    count.fill_(5)
    decay.fill_(0.999)
    raw = block.view(torch.uint8)
    assert bytes(raw[:8].tolist()) == (5).to_bytes(8, "little")
    assert raw[8:].view(torch.float64).item() == 0.999
    # the hyper block and the optimizer configuration are not touched by the feature
    assert int(_lib.lib().f3_optim_hyper_bytes()) == 72


def _aligned(t, align, skew=0):
    """The address of the first element of fp32 `t` at a multiple of `align` bytes, plus `skew` bytes."""
    base = t.data_ptr()
    return ctypes.c_void_p(base + (-base) % align + skew)


@pytest.mark.parametrize("bad", [-0.1, 1.5, float("nan"), float("inf"), -float("inf")])
def test_set_decay_refuses_a_bad_value_on_the_host(bad):
    """F3_EINVAL before anything touches the device: the block is host memory here, never dereferenced. A
    good value passes validation only on a device, so only the refusals are checked."""
    from fall_multimodal_amd import _lib
    L = _lib.lib()
    block = torch.zeros(8)
    assert L.f3_ema_set_decay(_aligned(block, 8), bad, None) == _lib.F3_EINVAL
    assert int(block.view(torch.int32).count_nonzero()) == 0


def test_set_decay_refuses_null_and_misaligned_blocks():
    from fall_multimodal_amd import _lib
    L = _lib.lib()
    block = torch.zeros(8)
    assert L.f3_ema_set_decay(None, 0.9, None) == _lib.F3_EINVAL
    assert L.f3_ema_set_decay(_aligned(block, 8, 4), 0.9, None) == _lib.F3_EINVAL


def test_update_refuses_bad_arguments_on_the_host():
    """NULL and misaligned pointers and n < 0: F3_EINVAL from host-side validation, with host pointers that
    are never dereferenced (the pattern of test_ranges_update_refuses_the_guard)."""
    from fall_multimodal_amd import _lib
    L = _lib.lib()
    a, b, s = torch.zeros(64), torch.zeros(64), torch.zeros(8)
    ema, par, st = _aligned(a, 16), _aligned(b, 16), _aligned(s, 8)
    E = _lib.F3_EINVAL
    assert L.f3_ema_update(None, par, 16, st, None) == E
    assert L.f3_ema_update(ema, None, 16, st, None) == E
    assert L.f3_ema_update(ema, par, 16, None, None) == E
    assert L.f3_ema_update(None, None, 0, st, None) == E  # n == 0 still needs its pointers
    for skew in (4, 8, 12):
        assert L.f3_ema_update(_aligned(a, 16, skew), par, 16, st, None) == E
        assert L.f3_ema_update(ema, _aligned(b, 16, skew), 16, st, None) == E
    assert L.f3_ema_update(ema, par, 16, _aligned(s, 8, 4), None) == E
    assert L.f3_ema_update(ema, par, -1, st, None) == E
    for t in (a, b, s):
        assert int(t.view(torch.int32).count_nonzero()) == 0


@pytest.mark.parametrize("good", [0, 1, 0.999, 0.0, 1.0])
def test_check_ema_decay_accepts(good):
    from fall_multimodal_amd.train import check_ema_decay
    v = check_ema_decay(good)
    assert isinstance(v, float) and v == float(good)


@pytest.mark.parametrize("bad", [True, False, "0.9", float("nan"), -0.1, 1.5, float("inf"), None, [0.9]])
def test_check_ema_decay_refuses(bad):
    from fall_multimodal_amd.train import check_ema_decay
    with pytest.raises(ValueError, match="ema_decay"):
        check_ema_decay(bad)


@pytest.mark.parametrize("bad", [True, "0.9", float("nan"), 2])
def test_trainstep_refuses_a_bad_decay_before_it_needs_a_model(bad):
    import fall_multimodal_amd as f3
    with pytest.raises(ValueError, match="ema_decay"):
        f3.TrainStep(None, 4, ema_decay=bad)


def test_trainstep_signature_and_surface():
    import fall_multimodal_amd as f3
    from fall_multimodal_amd.train import step_kwargs
    from fall_multimodal_amd.config import get_cfg_defaults
    sig = inspect.signature(f3.TrainStep.__init__)
    p = sig.parameters["ema_decay"]
    assert p.default is None and p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    prop = f3.TrainStep.ema_decay
    assert isinstance(prop, property) and prop.fset is not None
    for name in ("ema_update", "ema_state_dict", "swap_ema", "ema_checkpoint", "load_ema_checkpoint"):
        assert callable(getattr(f3.TrainStep, name)), name
    assert "ema_decay" not in step_kwargs(get_cfg_defaults())  # step_kwargs is as it was
