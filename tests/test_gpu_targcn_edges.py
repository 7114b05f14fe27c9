"""TARGCN step at edge shapes, gated tensor by tensor against the fp64 oracle (tests/targcn_ref.py).

Three modes per case: fp32, bf16 in the node-partitioned GRU form, and bf16 with F3_GN_NODE=0, which runs
the clip-tile GRU kernels (gru_fwd_kernel<true> / gru_bwd_kernel<true>: what a captured step or a batch past
the residency limit gets). What each shape is for:

  V=2,  B=1    one clip, two sequences: every tile ragged, fewer sequences than waves (idle waves must add
               zero to the workgroup reductions)
  V=16, B=5    exactly 16 nodes; 4+1 clips forward, 3+2 (bf16) or five single-clip (fp32) workgroups backward
  V=18, B=33   VMAX, and one clip past a full 32-clip barrier group
  V=17, B=65   three barrier groups (32, 32, 1); 1,105 sequences, more than 4 waves x 256 workgroups, so
               the attention kernels make a second, ragged pass; tg_supp_grad with rows / 4 not whole
  V=14, B=3    64 and 2 classes: head, loss and fc.2 gradient at both ends of the accepted class range

Every figure is appended to the parity record (tests.test_gpu_parity._record; the measured copy is kept as
profiles/targcn_edge_parity_record.jsonl).
"""
import numpy as np
import pytest
import torch

from tests import targcn_ref as R

pytestmark = pytest.mark.gpu

MODES = ["fp32", "bf16", "bf16_cliptile"]


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda")


def _run_step(d, case, mode, monkeypatch, poison=False, gn_node=None):
    """One TargcnStep at lr 1e-5 on the case's inputs: (logits, loss, {name: gradient})."""
    import fall_multimodal_amd as f3
    V, B, num_class = case
    if mode == "bf16_cliptile":
        gn_node = "0"
    if gn_node is not None:
        monkeypatch.setenv("F3_GN_NODE", gn_node)
    else:
        monkeypatch.delenv("F3_GN_NODE", raising=False)
    st, src, label = R.inputs(V, B, num_class)
    model = f3.TARGCN(num_nodes=V, num_classes=num_class, device=d, precision="fp32" if mode == "fp32" else "bf16")
    model.load_state_dict(st)
    step = f3.TargcnStep(model, B, lr=1e-5)
    if poison:
        step.ws.fill_(0xFF)
    step(torch.from_numpy(src).to(d), torch.from_numpy(label).to(d))
    model.device_status(wait=True)
    out = step.out.cpu().numpy().astype(np.float64)
    grads = {n: p.grad.detach().cpu().numpy().astype(np.float64) for n, p in model.named_parameters()}
    return out, float(step.loss.item()), grads


def _check(case, mode, out, loss, grads, test):
    """Record every figure, then gate logits, loss and every gradient against the fp64 oracle."""
    from tests.test_gpu_parity import _record
    V, B, num_class = case
    r64, env, tol, left_out, dl_emul = R.bf16_reference(*case)
    g64 = r64["grads"]
    assert len(g64) == 49 and set(grads) == set(g64)
    rat = R.ratios(grads, g64)
    cos = R.cosine(grads, g64)
    err = float(np.abs(out - r64["out"]).max())
    agree = float((out.argmax(1) == r64["out"].argmax(1)).mean())
    worst = max(rat, key=rat.get)
    over = {k: rat[k] / max(env[k], 1e-30) for k in g64}
    worst_env = max(tol, key=lambda k: over[k])
    print(f"TARGCN edge V={V} B={B} C={num_class} {mode}: max|dlogit| {err:.3e} (emulated {dl_emul:.3e}), argmax "
          f"agreement {agree:.4f}, loss {loss:.6f} vs {r64['loss']:.6f}, cosine {cos:.7f}, worst ratio "
          f"{rat[worst]:.3e} ({worst}), worst gated ratio/env {over[worst_env]:.2f} ({worst_env}), left out {left_out}")
    _record(test, {"V": V, "B": B, "num_class": num_class, "mode": mode, "max_abs_dlogit": err,
                   "emulated_max_abs_dlogit": dl_emul, "argmax_agreement": agree, "loss": loss, "loss_ref": r64["loss"],
                   "grad_cosine": cos, "worst_ratio": [worst, rat[worst]],
                   "worst_gated_ratio_over_env": [worst_env, over[worst_env]], "left_out": left_out,
                   "ratio": rat, "env": env, "ratio_over_env": over})
    assert np.isfinite(out).all() and np.isfinite(loss) and all(np.isfinite(g).all() for g in grads.values())
    if mode == "fp32":
        assert err <= R.FP32_LOGIT_TOL and agree == 1.0, (err, agree)
        assert abs(loss - r64["loss"]) <= R.FP32_LOSS_TOL
        R.gate(grads, g64, R.FP32_GRAD_TOL, what=f"{case} {mode}")
    else:
        assert err <= 4 * dl_emul and agree >= 0.99, (err, dl_emul, agree)
        assert abs(loss - r64["loss"]) <= 1e-3
        assert cos >= 0.999, cos
        R.gate(grads, g64, tol, what=f"{case} {mode}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "V%d-B%d-C%d" % c)
def test_targcn_edge_step_vs_fp64(case, mode, monkeypatch):
    """fp32: logits and loss within 1e-5 of the fp64 oracle with identical argmax, every gradient within
    1e-4 of its tensor's max. bf16, both GRU forms: every gated gradient within 4 x max(env_k, median env)
    of its tensor's max, env the fp64 oracle's own response to bf16 operand rounding (at most 4 tensors
    with a bound over 0.25 left to the cosine); logits within 4 x the emulated max|dlogit|, argmax
    agreement >= 0.99, loss within 1e-3, gradient cosine >= 0.999."""
    d = dev()
    out, loss, grads = _run_step(d, case, mode, monkeypatch)
    _check(case, mode, out, loss, grads, "targcn_edge_parity")


def test_gn_node_switch_selects_the_clip_tile_form(monkeypatch):
    """F3_GN_NODE=0 must really change the GRU kernels, or the bf16_cliptile cases above would run the
    node form twice: the two forms sum in different orders, so their logits at V=18, B=33 differ in some
    bit (measured max|dlogit| vs fp64 1.564e-4 and 1.588e-4) while both pass the gates above. Any other
    value of the variable leaves the node form on, bit for bit."""
    d = dev()
    case = (18, 33, 11)
    node, _, _ = _run_step(d, case, "bf16", monkeypatch)
    tile, _, _ = _run_step(d, case, "bf16_cliptile", monkeypatch)
    assert not np.array_equal(node, tile)
    on, _, _ = _run_step(d, case, "bf16", monkeypatch, gn_node="1")  # (the forward has no atomics)
    assert np.array_equal(on, node)


@pytest.mark.parametrize("mode", MODES)
def test_targcn_step_ignores_workspace_contents(mode, monkeypatch):
    """The step must not read a workspace byte it did not write: _SideStep allocates ws with torch.empty,
    which is usually zero in a fresh process and garbage in a long-running one. Every byte is set to 0xFF
    (NaN as fp32 and as bf16) before one step at V=18, B=33 (a ragged last barrier group, ragged clip
    tiles); logits, loss and gradients must be finite and pass the gates of the clean run. The barrier
    counters and the flag word are zeroed by the calls that use them (the forward clears all of them,
    each node-partitioned launch its own counters again), so the poison cannot reach a barrier."""
    d = dev()
    case = (18, 33, 11)
    out, loss, grads = _run_step(d, case, mode, monkeypatch, poison=True)
    _check(case, mode, out, loss, grads, "targcn_poisoned_workspace")
