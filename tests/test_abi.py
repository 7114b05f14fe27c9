"""C-ABI checks that need no GPU: libfall3.so loads, exports every function include/fall3.h
declares, and its host-side state_dict table (f3_net_create / f3_net_entry, no device
work) matches the reference's parameter names, shapes and order (oracle.param_shapes,
itself pinned to the reference's param-count golden vectors)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  (shared HIP runtime before the CDLL)

from oracle import model_cpu as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fall3.h")


def header_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(f3_\w+)\s*\(", src)))


def test_header_declares_the_boundary():
    fns = header_functions()
    for name in ("f3_net_create", "f3_net_forward", "f3_net_loss", "f3_net_backward", "f3_rmsprop_step"):
        assert name in fns


def test_library_exports_every_declared_symbol():
    import fall_multimodal_amd._lib as L
    so = ctypes.CDLL(L.LIB_PATH)
    missing = [f for f in header_functions() if not hasattr(so, f)]
    assert not missing, f"declared in fall3.h but not exported: {missing}"
    assert sorted(L.EXPORTS) == header_functions(), "_lib.EXPORTS out of sync with fall3.h"
    L.lib()  # every signature binds


def test_status_strings():
    import fall_multimodal_amd._lib as L
    for st in (L.F3_OK, L.F3_EINVAL, L.F3_EBATCH, L.F3_EHIP, L.F3_ESTATE):
        assert L.lib().f3_status_string(st)
    with pytest.raises(ValueError):
        L.check(L.F3_EBATCH, "x")
    with pytest.raises(RuntimeError):
        L.check(L.F3_EINVAL, "x")


SPECS = [
    oc.Spec(model="two_stgcan_bilstm", layout="coco_cut", num_class=11, sensor_dim=15),
    oc.Spec(model="two_stgcan_bilstm", layout="coco_mmpose", num_class=11, sensor_dim=6),
    oc.Spec(model="two_stgcan", layout="coco_cut", num_class=11),
    oc.Spec(model="stgcn", layout="coco_cut", strategy="spatial", num_class=11, in_channels=3),
    oc.Spec(model="bilstm", num_class=11, sensor_dim=15),
    oc.Spec(model="two_stgcan_bilstm", layout="coco_cut", num_class=2, sensor="cnn_bilstm", sensor_dim=4,
            sensor_classes=2, softmax_output=True, naming="notebook"),
    oc.Spec(model="bilstm", num_class=2, sensor="cnn_bilstm", sensor_dim=4),  # BASELINE config 1
]


@pytest.mark.parametrize("spec", SPECS, ids=lambda s: f"{s.model}-{s.layout}-{s.naming}-{s.sensor}")
@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
def test_entry_table_matches_reference_state_dict(spec, precision):
    from fall_multimodal_amd.graph import STRATEGY_PARTITIONS
    from fall_multimodal_amd.model import NativeNet, NetSpec
    ns = NetSpec(model=spec.model, layout=spec.layout, strategy=spec.strategy, num_class=spec.num_class,
                 in_channels=spec.in_channels, sensor=spec.sensor, sensor_dim=spec.sensor_dim,
                 sensor_classes=spec.sensor_classes, softmax_output=spec.softmax_output, naming=spec.naming,
                 precision=precision)
    V = 18 if spec.layout == "coco_mmpose" else 14
    net = NativeNet(ns, STRATEGY_PARTITIONS[spec.strategy], V)
    ref = oc.param_shapes(spec)
    got = [(n, tuple(sh)) for n, kind, sh, off in net.entries]
    assert [n for n, _ in got] == list(ref.keys())
    for n, sh in got:
        assert sh == tuple(ref[n]), n
    assert net.workspace_bytes(8) > 0


@pytest.mark.parametrize("name", ["two_stgcan_bilstm", "two_stgcan", "stgcn"])
def test_build_model_one_argument_call_is_bf16x3(name, monkeypatch):
    """The reference's driver calls build_model(config) with ONE argument (model/main.py:277,
    build_model.py:5-19); with only the reference's config keys that call must reach the benchmarked
    bf16x3 mode, read back from the native handle (f3_net_precision), and F3_PRECISION still selects
    the others. No device work: the module is built on the CPU (f3_net_create is host-only)."""
    import fall_multimodal_amd as f3
    import fall_multimodal_amd._lib as L
    from fall_multimodal_amd.config import get_cfg_defaults
    monkeypatch.delenv("F3_PRECISION", raising=False)
    cfg = get_cfg_defaults()
    cfg.merge_from_dict({"MODEL": {"NAME": name}, "GRAPH": {"LAYOUT": "coco_mmpose", "STRATEGY": "spatial"},
                         "DATA": {"NUM_CLASSES": 11, "SENSOR_DIM": 6}})
    model = f3.build_model(cfg, device="cpu")
    assert model.precision == "bf16x3" and model.spec.precision is None
    assert L.lib().f3_net_precision(model._native.h) == 4          # F3_PRECISION_BF16X3
    assert L.lib().f3_net_fused_rmsprop(model._native.h) == 1      # per-layer RMSprop plan holds
    monkeypatch.setenv("F3_PRECISION", "fp32")
    assert L.lib().f3_net_precision(f3.build_model(cfg, device="cpu")._native.h) == 0
    monkeypatch.setenv("F3_PRECISION", "fp8")
    with pytest.raises(ValueError):
        f3.build_model(cfg, device="cpu")


def test_bad_precision_rejected():
    from fall_multimodal_amd.model import NativeNet, NetSpec
    with pytest.raises(ValueError):
        NativeNet(NetSpec(precision="fp8"), 3, 14)


@pytest.mark.parametrize("spec", SPECS, ids=lambda s: f"{s.model}-{s.layout}-{s.naming}-{s.sensor}")
def test_param_offsets_tile_flat_buffer_phase1_first(spec):
    """Parameter offsets tile [0, nparam) in order, each entry 16-B aligned with < 4 floats of
    padding after it (float4 RMSprop); the gradients final after backward phase 1
    (head, sensor, skeleton layers >= 4 and their edge_importance) occupy [0, grad_split)."""
    import fall_multimodal_amd._lib as L
    from fall_multimodal_amd.graph import STRATEGY_PARTITIONS
    from fall_multimodal_amd.model import NativeNet, NetSpec
    ns = NetSpec(model=spec.model, layout=spec.layout, strategy=spec.strategy, num_class=spec.num_class,
                 in_channels=spec.in_channels, sensor=spec.sensor, sensor_dim=spec.sensor_dim,
                 sensor_classes=spec.sensor_classes, softmax_output=spec.softmax_output, naming=spec.naming)
    V = 18 if spec.layout == "coco_mmpose" else 14
    net = NativeNet(ns, STRATEGY_PARTITIONS[spec.strategy], V)
    split = L.lib().f3_net_grad_split(net.h)
    spans = sorted((off, off + int(np.prod(sh)), n) for n, kind, sh, off in net.entries if kind == L.ENTRY_PARAM)
    pos = 0
    for a, b, n in spans:
        assert a % 4 == 0 and pos <= a < pos + 4, n
        pos = b
    assert pos <= net.nparam < pos + 4 and net.nparam % 4 == 0
    assert 0 < split <= net.nparam
    for a, b, n in spans:
        m = re.search(r"(?:st_gc[a]?n_networks|edge_importance)\.(\d+)", n)
        phase1 = (m is None and "data_bn" not in n) or (m is not None and int(m.group(1)) >= 4)
        assert (b <= split) == phase1, n


@pytest.mark.parametrize("V", [14, 17, 18])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_targcn_entry_table_matches_reference_state_dict(V, precision):
    """f3_targcn_entry: TARGCN(adj=None, num_nodes=V)'s exact state_dict keys, order and shapes
    (TRAGCN.py:177-205; pinned by the oracle's table and the reference's parameter counts), 16-B
    aligned parameter offsets, positive workspace."""
    from oracle import targcn_cpu as tg
    from fall_multimodal_amd.targcn import _NativeTargcn
    net = _NativeTargcn(V, 11, precision)
    ref = tg.param_shapes(V)
    assert [n for n, k, sh, off in net.entries] == list(ref.keys())
    for n, kind, sh, off in net.entries:
        assert tuple(sh) == tuple(ref[n]), n
        assert (kind == 1) == tg.is_buffer(n), n
        if kind == 0:
            assert off % 4 == 0, n
    assert net.workspace_bytes(256) > net.workspace_bytes(4) > 0


def test_targcn_rejects_unsupported_configs():
    from fall_multimodal_amd.targcn import TARGCN, _NativeTargcn
    with pytest.raises(RuntimeError):
        _NativeTargcn(40, 11, "fp32")  # beyond the per-tile LDS layout (V <= 18)
    with pytest.raises(ValueError):
        _NativeTargcn(14, 11, "fp8")
    with pytest.raises(NotImplementedError):
        TARGCN(rnn_units=32, device="cpu")
    with pytest.raises(ValueError):
        TARGCN(adj=np.ones((14, 14)), device="cpu")


def test_custom_ops_registered_with_fake_kernels():
    """the native step is reachable as torch.library custom ops with fake kernels,
    so shapes propagate under FakeTensor tracing (torch.compile) without a device."""
    import torch
    from torch._subclasses import FakeTensorMode
    import fall_multimodal_amd as f3
    for op in ("net_forward", "net_backward", "targcn_forward", "targcn_backward", "sktr_forward", "sktr_backward",
               "musa_forward", "musa_backward", "rmsprop_"):
        assert hasattr(torch.ops.fall3, op), op
    m = f3.TwoStreamSTGCAN_BiLSTM(3, {"layout": "coco_mmpose", "strategy": "spatial"}, 11, 6, device="cpu")
    t = f3.TARGCN(num_nodes=17, device="cpu")
    with FakeTensorMode(allow_non_fake_inputs=True):
        out, ws, nb, nc = torch.ops.fall3.net_forward(m._op_id, list(m.parameters()), m._flat_buffers,
                                                      m._flat_counters, torch.empty(8, 3, 30, 18),
                                                      torch.empty(8, 30, 6), True)
        assert tuple(out.shape) == (8, 11) and ws.numel() == m._native.workspace_bytes(8)
        assert nb.shape == m._flat_buffers.shape and nc.shape == m._flat_counters.shape
        g = torch.ops.fall3.net_backward(m._op_id, list(m.parameters()), out, ws)
        assert g.numel() == m._native.nparam
        o2, w2 = torch.ops.fall3.targcn_forward(t._op_id, list(t.parameters()), t._flat_buffers,
                                                torch.empty(4, 30, 17, 3))
        assert tuple(o2.shape) == (4, 11) and w2.numel() == t._native.workspace_bytes(4)
        k = f3.SkeletonTransformer(device="cpu")
        o3, w3, b3, c3 = torch.ops.fall3.sktr_forward(k._op_id, list(k.parameters()), k._flat_buffers, k._counters,
                                                      torch.empty(6, 3, 30, 14, 1), True, [1.0] * 18, 7)
        assert tuple(o3.shape) == (6, 11) and w3.numel() == k._native.workspace_bytes(6)
        assert torch.ops.fall3.sktr_backward(k._op_id, list(k.parameters()), o3, w3).numel() == k._native.nparam
        u = f3.musa.Model(11, 14, 300, f3.musa.adjGraph("coco_cut", "uniform"), True, True, 41, device="cpu")
        o4, w4, b4, c4 = torch.ops.fall3.musa_forward(u._op_id, list(u.parameters()), u._flat_buffers, u._counters,
                                                      torch.empty(5, 3, 30, 14), True, 7)
        assert tuple(o4.shape) == (5, 11) and w4.numel() == u._native.workspace_bytes(5)
        assert b4.shape == u._flat_buffers.shape and c4.shape == u._counters.shape and c4.dtype == torch.int64
        assert torch.ops.fall3.musa_backward(u._op_id, list(u.parameters()), o4, w4).numel() == u._native.nparam


@pytest.mark.parametrize("V,T,M", [(14, 30, 1), (17, 30, 2), (18, 32, 1)])
def test_sktr_entry_table_matches_reference_state_dict(V, T, M):
    """f3_sktr_entry: SkeletonTransformer(3, V, T, 11, 32, 6, 16, 8)'s exact state_dict keys, order and
    shapes (skeleton_transformer.py:360-416, checked against the reference module by
    tools/gen_golden.py), 262,091 parameters at V=14/T=30, 16-B aligned parameter offsets, BatchNorm3d
    running statistics as buffers and num_batches_tracked as int64 counters."""
    from oracle import sktr_cpu as sk
    from fall_multimodal_amd.sktr import _NativeSktr
    net = _NativeSktr(V, T, M, 11)
    ref = sk.param_shapes(V, T)
    assert [n for n, k, sh, off in net.entries] == list(ref.keys())
    nparam = 0
    for n, kind, sh, off in net.entries:
        assert tuple(sh) == tuple(ref[n]), n
        if n.endswith("num_batches_tracked"):
            assert kind == 2, n
        else:
            assert (kind == 1) == sk.is_buffer(n), n
        if kind == 0:
            assert off % 4 == 0, n
            nparam += int(np.prod(sh))
    if (V, T) == (14, 30):
        assert nparam == 262091
    assert net.ncnt == 18 and net.nbuf == 18 * 2 * 32
    assert net.workspace_bytes(64) > net.workspace_bytes(4) > 0


def test_musa_entry_table_matches_reference_state_dict():
    """f3_musa_entry: musa_model.Model's exact state_dict keys, order and shapes (checked against the
    reference module by tools/gen_golden.py), 427,107 trainable parameters (+ the frozen A)."""
    from oracle import musa_cpu as mu
    from fall_multimodal_amd.musa import _NativeMusa
    net = _NativeMusa(14, 30, 11)
    ref = mu.param_shapes()
    assert [n for n, k, sh, off in net.entries] == list(ref.keys())
    n_train = 0
    for n, kind, sh, off in net.entries:
        assert tuple(sh) == tuple(ref[n]), n
        assert kind == (2 if n.endswith("num_batches_tracked") else 1 if mu.is_buffer(n) else 0), n
        if kind == 0:
            assert off % 4 == 0
            if not mu.is_frozen(n):
                n_train += int(np.prod(sh))
    assert n_train == 427107 and net.ncnt == 22
    assert net.workspace_bytes(64) > net.workspace_bytes(4) > 0


def test_sktr_rejects_unsupported_configs():
    from fall_multimodal_amd.sktr import SkeletonTransformer, _NativeSktr
    with pytest.raises(RuntimeError):
        _NativeSktr(20, 30, 1, 11)   # attention length without a compiled kernel
    with pytest.raises(RuntimeError):
        _NativeSktr(14, 30, 0, 11)
    with pytest.raises(NotImplementedError):
        SkeletonTransformer(embedding_dim=64, device="cpu")
