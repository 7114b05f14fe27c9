"""The flat-storage base (fall_multimodal_amd/_flat.py) under the four native-backed models, on the CPU
with the built library (f3_*_create and the entry table are host-only): registration order, aliasing
into the flat arrays, re-flattening in .to() / .float() / .double(), frozen parameters and the order
in which the constructors draw from the torch RNG."""
import pytest
import torch

ENTRY_PARAM, ENTRY_BUFFER, ENTRY_COUNTER = 0, 1, 2


def _fall3():
    import fall_multimodal_amd as f3
    return f3.TwoStreamSTGCAN_BiLSTM(3, {"layout": "coco_mmpose", "strategy": "spatial"}, 11, 6, device="cpu")


def _notebook():
    import fall_multimodal_amd as f3
    return f3.TwoStreamSpatialTemporalGraph({"layout": "coco_cut", "strategy": "spatial"}, 11, device="cpu")


def _targcn():
    import fall_multimodal_amd as f3
    return f3.TARGCN(num_nodes=17, device="cpu")


def _sktr():
    import fall_multimodal_amd as f3
    return f3.SkeletonTransformer(device="cpu")


def _musa():
    from fall_multimodal_amd import musa
    return musa.Model(11, 14, 300, musa.adjGraph("coco_cut", "uniform"), True, True, 41, device="cpu")


MODELS = {"fall3": _fall3, "fall3_notebook": _notebook, "targcn": _targcn, "sktr": _sktr, "musa": _musa}
# the attribute each class has always kept its int64 counter array under (TARGCN has none)
COUNTERS = {"fall3": "_flat_counters", "fall3_notebook": "_flat_counters", "targcn": None, "sktr": "_counters",
            "musa": "_counters"}


def check_order_and_aliasing(m, counters_attr):
    """state_dict order = entry-table order, named_parameters order = param_views order, and every
    tensor is a view of the flat array of its kind at its entry's offset."""
    entries = m._native.entries
    sd = m.state_dict()
    assert list(sd.keys()) == [n for n, _, _, _ in entries]
    named = list(m.named_parameters())
    views = m.param_views()
    assert [n for n, _ in named] == [n for n, _, _ in views]
    assert views == [(n, s, o) for n, k, s, o in entries if k == ENTRY_PARAM]
    flat = m.flat_parameters()
    assert flat is m._flat_params and flat.dtype == torch.float32 and flat.numel() == m._native.nparam
    for (name, p), (_, shape, off) in zip(named, views):
        assert isinstance(p, torch.nn.Parameter) and tuple(p.shape) == tuple(shape), name
        assert p.dtype == torch.float32 and p.is_contiguous(), name
        assert p.data_ptr() == flat.data_ptr() + 4 * off, name
    buffers = dict(m.named_buffers())
    counters = getattr(m, counters_attr) if counters_attr else None
    if counters is not None:
        assert counters.dtype == torch.int64
    assert (counters is not None) or not any(k == ENTRY_COUNTER for _, k, _, _ in entries)
    for name, kind, shape, off in entries:
        if kind == ENTRY_PARAM:
            continue
        b = buffers[name]
        assert tuple(b.shape) == tuple(shape) and sd[name].data_ptr() == b.data_ptr(), name
        if kind == ENTRY_BUFFER:
            assert b.dtype == torch.float32 and b.data_ptr() == m._flat_buffers.data_ptr() + 4 * off, name
        else:
            assert b.dtype == torch.int64 and b.data_ptr() == counters.data_ptr() + 8 * off, name


@pytest.mark.parametrize("kind", list(MODELS))
def test_order_and_aliasing_fresh_and_after_to(kind):
    m = MODELS[kind]()
    check_order_and_aliasing(m, COUNTERS[kind])
    assert m.to("cpu") is m
    check_order_and_aliasing(m, COUNTERS[kind])


@pytest.mark.parametrize("kind", list(MODELS))
def test_to_keeps_parameters_and_values_in_new_storage(kind):
    m = MODELS[kind]()
    with torch.no_grad():  # a non-default counter and running statistic must survive too
        for name, b in m.named_buffers():
            b.copy_(torch.arange(b.numel(), dtype=b.dtype).view(b.shape) + 3)
    before = list(m.parameters())
    values = {k: v.clone() for k, v in m.state_dict().items()}
    old_flat, old_ptr = m.flat_parameters(), m.flat_parameters().data_ptr()
    old_bits = old_flat.clone()
    m.to("cpu")
    m.float()
    after = list(m.parameters())
    assert len(after) == len(before) and all(a is b for a, b in zip(after, before))
    assert m.flat_parameters() is not old_flat and m.flat_parameters().data_ptr() != old_ptr
    assert torch.equal(m.flat_parameters().view(torch.int32), old_bits.view(torch.int32))
    sd = m.state_dict()
    assert list(sd.keys()) == list(values.keys())
    for k, v in values.items():
        assert sd[k].dtype == v.dtype and torch.equal(sd[k], v), k
    with torch.no_grad():  # the old array is no longer what the parameters alias
        old_flat.add_(1.0)
    assert torch.equal(m.flat_parameters().view(torch.int32), old_bits.view(torch.int32))


@pytest.mark.parametrize("kind", list(MODELS))
def test_double_keeps_fp32_storage(kind):
    m = MODELS[kind]()
    bits = m.flat_parameters().clone()
    m.double()
    assert m.flat_parameters().dtype == torch.float32 and m._flat_buffers.dtype == torch.float32
    assert all(p.dtype == torch.float32 for p in m.parameters())
    assert all(b.dtype in (torch.float32, torch.int64) for b in m.buffers())
    assert torch.equal(m.flat_parameters().view(torch.int32), bits.view(torch.int32))
    check_order_and_aliasing(m, COUNTERS[kind])


@pytest.mark.parametrize("kind", list(MODELS))
def test_requires_grad_false_exactly_for_musa_graphs(kind):
    m = MODELS[kind]()
    frozen = [n for n, p in m.named_parameters() if not p.requires_grad]
    if kind == "musa":
        want = [n for n, _, _ in m.param_views() if n == "A" or n.endswith(".A")]
        assert want and frozen == want
    else:
        assert frozen == []
    m.to("cpu")
    assert [n for n, p in m.named_parameters() if not p.requires_grad] == frozen


@pytest.mark.parametrize("kind", list(MODELS))
def test_same_seed_same_initial_weights(kind):
    torch.manual_seed(5)
    a = MODELS[kind]()
    after_a = torch.rand(1)
    torch.manual_seed(5)
    b = MODELS[kind]()
    after_b = torch.rand(1)
    assert torch.equal(a.flat_parameters(), b.flat_parameters())
    assert torch.equal(after_a, after_b)  # the same number of draws
    assert a.flat_parameters().data_ptr() != b.flat_parameters().data_ptr()
    torch.manual_seed(6)
    assert not torch.equal(MODELS[kind]().flat_parameters(), a.flat_parameters())


@pytest.mark.parametrize("kind", list(MODELS))
def test_split_grads_table_is_cached_on_the_module(kind):
    """ops._split_grads: views of a flat gradient at the parameter offsets; its table is built once."""
    from fall_multimodal_amd import ops
    m = MODELS[kind]()
    g = torch.arange(m._native.nparam, dtype=torch.float32)
    views = ops._split_grads(m, g)
    table = m._f3_grad_table
    assert ops._split_grads(m, g) is not None and m._f3_grad_table is table
    for v, p, (_, shape, off) in zip(views, m.parameters(), m.param_views()):
        assert v.shape == p.shape and v.data_ptr() == g.data_ptr() + 4 * off
