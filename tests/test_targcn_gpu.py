"""TARGCN (BASELINE config 2) HIP path vs the reference's golden vectors and the CPU oracle.

Golden fixtures come from the reference's own TARGCN(adj=None) (tools/gen_golden.py); the oracle
(oracle/targcn_cpu.py) is pinned bit-exactly to them by tests/test_oracle_golden.py.
"""
import os

import numpy as np
import pytest
import torch

from oracle import targcn_cpu as tg
from tests.golden_util import GOLDEN, check_packed

pytestmark = pytest.mark.gpu


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda")


def _golden(tag):
    z = np.load(os.path.join(GOLDEN, f"targcn_{tag}.npz"))
    return {k: z[k] for k in z.files}


def _grad_rel(ours, ref):
    ours, ref = np.asarray(ours, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    return float(np.abs(ours - ref).max() / max(np.abs(ref).max(), 1e-30))


@pytest.mark.parametrize("tag", ["v14", "v17"])
def test_targcn_train_step_matches_reference_golden(tag):
    """fp32 mode vs the reference's own outputs (B=3-4): logits within 1e-3 with identical argmax
    (north-star gate), loss within 1e-5, every gradient within 1e-3 of its tensor's max |g| (no
    batch statistics in this model, so gradients are well conditioned), RMSprop(lr=1e-5) update."""
    d = dev()
    import fall_multimodal_amd as f3
    g = _golden(tag)
    V = int(g["V"][0])
    st = tg.init_state(V, int(g["seed"][0]))
    model = f3.TARGCN(num_nodes=V, device=d)
    model.load_state_dict(st, strict=True)
    src = torch.from_numpy(g["source"]).to(d)
    label = torch.from_numpy(g["label"]).to(d)
    out = model(src)
    o = out.detach().cpu().numpy()
    err = float(np.abs(o - g["out"]).max())
    assert err < 1e-3, err
    assert (o.argmax(1) == g["out"].argmax(1)).all()
    loss = torch.nn.CrossEntropyLoss()(out, label)
    np.testing.assert_allclose(loss.item(), g["loss"][0], rtol=0, atol=1e-5)
    opt = f3.RMSprop(model.parameters(), lr=float(g["lr"][0]))
    opt.zero_grad()
    loss.backward()
    worst = {}
    for name, p in model.named_parameters():
        gr = p.grad.detach().cpu().numpy()
        check_packed(g, "grad:" + name, gr, rtol=1e-3, atol=1e-3 * float(np.abs(gr).max()) + 1e-9, what=tag + " ")
        if "grad:" + name in g:
            worst[name] = _grad_rel(gr, g["grad:" + name])
    print(f"{tag}: max|dlogit| {err:.2e}; worst full-tensor grad rel err "
          f"{max(worst.values()):.2e} ({max(worst, key=worst.get)})")
    opt.step()
    for name, p in model.named_parameters():
        check_packed(g, "post:" + name, p.detach().cpu().numpy(), rtol=1e-5, atol=2e-7, what=tag + " ")


def _oracle_grads(st, src, label):
    out, loss, grads = tg.train_step({k: v.clone() for k, v in st.items()}, torch.from_numpy(src),
                                     torch.from_numpy(label))
    return out.numpy(), loss.item(), grads


@pytest.mark.parametrize("precision,B", [("fp32", 40), ("bf16", 40), ("bf16", 256)])
def test_targcn_step_vs_oracle(precision, B):
    """TargcnStep (native fwd + CE + bwd + RMSprop) vs the oracle on a ragged multi-tile batch.
    fp32: logits 1e-3 / identical argmax / every gradient within 2e-3 of its max (measured
    4.5e-8 / 2e-6). bf16 (GEMM operands bf16, fp32 accumulate and state, the TA layers' products too, on
    bf16 MFMA): logits within 5e-3, argmax agreement >= 0.99, cosine >= 0.999 against the fp32 oracle, and
    every gradient gated on its own against the fp64 oracle (tests/targcn_ref.py): within
    4 x max(env_k, median env) of its tensor's max, env the fp64 oracle's own response to bf16 operand
    rounding, a bound over 0.25 leaving the tensor to the cosine (none at these shapes). Both fp64 runs
    of B=256 take about 3 s each on 16 threads and are cached, so B=40 and B=256 are both gated. The
    measured values are in profiles/targcn_edge_parity_record.jsonl (test "targcn_bf16_parity")."""
    d = dev()
    import fall_multimodal_amd as f3
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    V = 17
    st = tg.init_state(V, 11)
    src, label = tg.synthetic_source(B, V, 11, 5)
    model = f3.TARGCN(num_nodes=V, device=d, precision=precision)
    model.load_state_dict(st)
    step = f3.TargcnStep(model, B, lr=1e-5)
    step(torch.from_numpy(src).to(d), torch.from_numpy(label).to(d))
    out_ref, loss_ref, grads_ref = _oracle_grads(st, src, label)
    out = step.out.cpu().numpy()
    err = float(np.abs(out - out_ref).max())
    agree = float((out.argmax(1) == out_ref.argmax(1)).mean())
    ours = {n: p.grad.detach().cpu().numpy() for n, p in model.named_parameters()}
    a = np.concatenate([ours[k].reshape(-1) for k in grads_ref]).astype(np.float64)
    r = np.concatenate([grads_ref[k].numpy().reshape(-1) for k in grads_ref]).astype(np.float64)
    cos = float(a @ r / (np.linalg.norm(a) * np.linalg.norm(r)))
    rel = {k: _grad_rel(ours[k], grads_ref[k].numpy()) for k in grads_ref}
    worst = max(rel, key=rel.get)
    print(f"TARGCN {precision} B={B}: max|dlogit| {err:.3e}, argmax agreement {agree:.4f}, grad cosine {cos:.6f}, "
          f"worst grad rel {rel[worst]:.2e} ({worst}), loss {step.loss.item():.6f} vs {loss_ref:.6f}")
    if precision == "fp32":
        assert err < 1e-3 and agree == 1.0
        assert rel[worst] < 2e-3, (worst, rel[worst])
        assert abs(step.loss.item() - loss_ref) < 1e-5
    else:
        from tests import targcn_ref as R
        from tests.test_gpu_parity import _record
        r64, env, tol, left_out, _ = R.bf16_reference(V, B, 11, 11, 5)
        rat = R.ratios(ours, r64["grads"])
        over = {k: rat[k] / max(env[k], 1e-30) for k in rat}
        worst_env = max(tol, key=lambda k: over[k])
        print(f"TARGCN bf16 B={B} vs fp64: worst gated ratio/env {over[worst_env]:.2f} ({worst_env}), left out {left_out}")
        _record("targcn_bf16_parity", {"B": B, "max_abs_dlogit": err, "argmax_agreement": agree, "grad_cosine": cos,
                                       "worst_grad_rel": [worst, rel[worst]], "loss": float(step.loss.item()),
                                       "loss_ref": float(loss_ref),
                                       "worst_gated_ratio_over_env": [worst_env, over[worst_env]],
                                       "left_out": left_out, "ratio_over_env": over})
        assert err < 5e-3 and agree >= 0.99
        assert cos >= 0.999
        assert abs(step.loss.item() - loss_ref) < 1e-3
        R.gate(ours, r64["grads"], tol, what=f"bf16 B={B}")


def test_targcn_training_tracks_oracle():
    """Six RMSprop steps (lr 1e-4) on cycled batches: the fp32 HIP path follows the oracle's loss
    trajectory (1e-4) and the trained models agree on held-out clips (logits within 1e-3, same
    argmax). Parameters are not compared elementwise: RMSprop moves an element by up to 10*lr on
    its first step whatever its gradient size (v = 0.01 g^2), so elements whose gradient is at
    rounding level move differently in any two implementations (measured: per-tensor relative L2
    up to 2.7e-3 on weights_pool, whose entries are ~1e-2)."""
    d = dev()
    import fall_multimodal_amd as f3
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    V, B, steps = 14, 24, 6
    st = tg.init_state(V, 21)
    batches = [tg.synthetic_source(B, V, 11, 40 + i) for i in range(3)]
    model = f3.TARGCN(num_nodes=V, device=d)
    model.load_state_dict(st)
    step = f3.TargcnStep(model, B, lr=1e-4)
    ref = {k: v.clone() for k, v in st.items()}
    sq = None
    for i in range(steps):
        src, lab = batches[i % 3]
        loss = step(torch.from_numpy(src).to(d), torch.from_numpy(lab).to(d)).item()
        if sq is None:
            sq = {k: torch.zeros_like(v) for k, v in ref.items() if not tg.is_buffer(k)}
        _, loss_ref, _ = tg.train_step(ref, torch.from_numpy(src), torch.from_numpy(lab), lr=1e-4, sq=sq)
        assert abs(loss - loss_ref.item()) < 1e-4, (i, loss, loss_ref.item())
    src, _ = tg.synthetic_source(64, V, 11, 99)
    with torch.no_grad():
        out = model(torch.from_numpy(src).to(d)).cpu().numpy()
        out_ref = tg.forward(ref, torch.from_numpy(src)).numpy()
    err = float(np.abs(out - out_ref).max())
    print(f"TARGCN after {steps} steps: held-out max|dlogit| {err:.2e}")
    assert err < 1e-3 and (out.argmax(1) == out_ref.argmax(1)).all()


def test_targcn_gru_barrier_timeout_is_reported(monkeypatch):
    """The node-partitioned GRU recurrences (bf16) synchronise a clip group's V workgroups with a
    bounded-spin barrier. A barrier that times out must surface as F3_EDEVICE, not as F3_OK with
    wrong logits: F3_GN_SKIP_ARRIVE=1 makes workgroup 0 skip its arrivals, and the step must then
    raise (from the native calls or from device_status). A clean step before and after reports OK
    (the flag is cleared per forward)."""
    d = dev()
    import fall_multimodal_amd as f3
    V, B = 17, 64
    st = tg.init_state(V, 11)
    src, label = (torch.from_numpy(x).to(d) for x in tg.synthetic_source(B, V, 11, 5))
    model = f3.TARGCN(num_nodes=V, device=d, precision="bf16")
    model.load_state_dict(st)
    step = f3.TargcnStep(model, B, lr=1e-5)
    step.forward_backward(src, label)
    model.device_status(wait=True)
    monkeypatch.setenv("F3_GN_SKIP_ARRIVE", "1")
    with pytest.raises(RuntimeError, match="barrier"):
        step.forward_backward(src, label)
        model.device_status(wait=True)
    monkeypatch.delenv("F3_GN_SKIP_ARRIVE")
    torch.cuda.synchronize()
    model.device_status(wait=True)  # the flagged word was consumed by the raise
    step.forward_backward(src, label)
    model.device_status(wait=True)
    assert np.isfinite(step.out.cpu().numpy()).all()


def test_targcn_backward_barrier_flag_survives_later_forward(monkeypatch):
    """a barrier timeout raised only in step k's BACKWARD must still be reported when the
    host runs ahead and submits step k+1's clean forward before asking (no sync in between): each
    call's flag copy lands in its own host word, so the later clean copy cannot overwrite it.
    F3_GN_SKIP_ARRIVE=2 skips the arrivals in the backward recurrences only."""
    d = dev()
    import fall_multimodal_amd as f3
    V, B = 17, 64
    st = tg.init_state(V, 11)
    src, label = (torch.from_numpy(x).to(d) for x in tg.synthetic_source(B, V, 11, 5))
    model = f3.TARGCN(num_nodes=V, device=d, precision="bf16")
    model.load_state_dict(st)
    step = f3.TargcnStep(model, B, lr=1e-5)
    step.forward_backward(src, label)
    model.device_status(wait=True)
    monkeypatch.setenv("F3_GN_SKIP_ARRIVE", "2")
    step.forward_backward(src, label)           # clean forward, faulting backward
    monkeypatch.delenv("F3_GN_SKIP_ARRIVE")
    raised = False
    try:
        m = step.model
        m.native_forward(src, step.out, step.ws, f3._lib.stream_handle())   # clean forward, no sync
        torch.cuda.synchronize()
    except RuntimeError:                        # the native call may already report it
        raised = True
    if not raised:
        with pytest.raises(RuntimeError):
            model.device_status(wait=True)
    torch.cuda.synchronize()
    model.device_status(wait=True)              # reported once, then clear
    step.forward_backward(src, label)
    model.device_status(wait=True)

