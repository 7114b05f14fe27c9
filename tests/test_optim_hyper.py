"""What a captured optimizer graph fixes and what it reads from the device hyper-parameter block, on the
host side (no GPU): optim.hyper_structure, and the three C entries in the header and in _lib.EXPORTS."""
import ctypes
import os
import re

import pytest

from fall_multimodal_amd import optim as fo

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fall3.h")

ADAM = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
RMS = dict(lr=1e-3, alpha=0.99, eps=1e-8)
SGD = dict(lr=1e-2, momentum=0.9, nesterov=False, weight_decay=0.0)

# (kind, group, max_norm) pairs a recorded graph serves alike: only values differ
EQUAL = [
    (("adam", ADAM, None), ("adam", dict(ADAM, lr=5e-4), None)),
    (("adam", ADAM, None), ("adam", dict(ADAM, betas=(0.8, 0.99), eps=1e-6), None)),
    (("adamw", ADAM, 1.0), ("adamw", dict(ADAM, weight_decay=0.05), 1.0)),
    (("adamw", ADAM, 1.0), ("adamw", ADAM, 0.25)),
    (("rmsprop", RMS, None), ("rmsprop", dict(RMS, lr=1e-5, alpha=0.9, eps=1e-6), None)),
    (("rmsprop", RMS, None), ("rmsprop", RMS, 0.0)),
    (("rmsprop", dict(RMS, weight_decay=0.01), None), ("rmsprop", dict(RMS, weight_decay=0.02, alpha=0.95), None)),
    (("sgd", SGD, None), ("sgd", dict(SGD, momentum=0.5, lr=1.0), None)),
    (("sgd", SGD, 2.0), ("sgd", dict(SGD, weight_decay=0.01), 3.0)),  # decay 0 <-> nonzero: same kernel off RMSprop
]
# pairs that need other launches or another kernel variant
DIFFERENT = [
    (("sgd", dict(SGD, momentum=0.0), None), ("sgd", SGD, None)),
    (("sgd", SGD, None), ("sgd", dict(SGD, nesterov=True), None)),
    (("rmsprop", RMS, None), ("rmsprop", dict(RMS, weight_decay=0.01), None)),
    (("rmsprop", RMS, None), ("rmsprop", RMS, 1.0)),
    (("adam", ADAM, None), ("adam", ADAM, 1.0)),
    (("adam", ADAM, 0.0), ("adam", ADAM, 0.5)),
    (("adam", ADAM, None), ("adamw", ADAM, None)),
    (("rmsprop", dict(RMS, weight_decay=0.01), None), ("adam", ADAM, None)),
]


@pytest.mark.parametrize("a,b", EQUAL)
def test_values_do_not_change_the_structure(a, b):
    assert fo.hyper_structure(*a) == fo.hyper_structure(*b)


@pytest.mark.parametrize("a,b", DIFFERENT)
def test_structure_changes_are_seen(a, b):
    assert fo.hyper_structure(*a) != fo.hyper_structure(*b)


def test_structure_key_fields():
    """(kind, nesterov, momentum != 0, legacy, max_norm > 0), one name per field for the error message."""
    assert fo.hyper_structure("rmsprop", RMS, None) == ("rmsprop", False, False, True, False)
    assert fo.hyper_structure("rmsprop", dict(RMS, weight_decay=0.01), 1.0) == ("rmsprop", False, False, False, True)
    assert fo.hyper_structure("sgd", dict(SGD, nesterov=True), None) == ("sgd", True, True, False, False)
    assert fo.hyper_structure("adamw", ADAM, 0.5) == ("adamw", False, False, False, True)
    assert len(fo.STRUCTURE_FIELDS) == 5
    # a momentum or nesterov key on a kind that has none is not structure
    assert fo.hyper_structure("adam", dict(ADAM, momentum=0.9, nesterov=True), None) == \
        fo.hyper_structure("adam", ADAM, None)


def test_header_and_exports_list_the_entries():
    from fall_multimodal_amd import _lib, ops
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("f3_optim_hyper_bytes", "f3_optim_hyper_set", "f3_optim_step_hyper"):
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    # the documented layout: nine fp64 values in f3_optim_config's order
    assert _lib.lib().f3_optim_hyper_bytes() == 8 * len(ops.HYPER_FIELDS) == 72
    cfg_doubles = [n for n, t in _lib.F3OptimConfig._fields_ if t is ctypes.c_double]
    assert tuple(cfg_doubles) == ops.HYPER_FIELDS
