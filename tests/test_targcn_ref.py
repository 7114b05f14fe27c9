"""CPU tests of the TARGCN gradient gate itself (tests/targcn_ref.py): the references run at the edge
shapes, the reference alone stays inside the cap, and a wrong gradient in any single gated tensor fails."""
import numpy as np
import pytest

from tests import targcn_ref as R

IDS = ["V%d-B%d-C%d" % c for c in R.CASES]


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_fp64_oracle_runs_and_fp32_oracle_passes_fp32_gate(case):
    """The fp64 step runs unchanged at every edge shape, and the oracle as written (fp32) passes the
    fp32-mode gate against it: gradients 1e-4, logits 1e-5 with identical argmax, loss 1e-5 (measured:
    gradients <= 6e-6, logits <= 8e-8, loss <= 2e-7)."""
    V, B, num_class = case
    r64, r32 = R.oracle_fp64(*case), R.oracle_fp32(*case)
    assert r64["out"].shape == (B, num_class) and len(r64["grads"]) == 49
    assert np.isfinite(r64["out"]).all() and np.isfinite(r64["loss"])
    assert all(np.isfinite(g).all() and np.abs(g).max() > 0 for g in r64["grads"].values())
    assert R.oracle_fp64(*case) is r64  # cached: the modes of one case share one run
    rat = R.gate(r32["grads"], r64["grads"], R.FP32_GRAD_TOL, what=str(case))
    err = float(np.abs(r32["out"] - r64["out"]).max())
    print(f"{case}: fp32 oracle vs fp64: worst gradient ratio {max(rat.values()):.2e}, max|dlogit| {err:.2e}")
    assert err <= R.FP32_LOGIT_TOL and (r32["out"].argmax(1) == r64["out"].argmax(1)).all()
    assert abs(r32["loss"] - r64["loss"]) <= R.FP32_LOSS_TOL


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_bf16_operand_run_stays_inside_cap(case):
    """The reference's own response to bf16 operand rounding leaves at most OVER_CAP[case] tensors with a
    bound over the cap (2 at V=2, B=1: ff.0 weight / bias, ReLU kinks with 2 sequences; none elsewhere),
    passes its own gate, and restores the oracle's functions."""
    from oracle import targcn_cpu as tg
    embgcn, transform = tg.embgcn, tg.transform
    r64, env, tol, left_out, dl = R.bf16_reference(*case)
    assert tg.embgcn is embgcn and tg.transform is transform
    med = float(np.median(list(env.values())))
    print(f"{case}: worst env {max(env.values()):.4f} ({max(env, key=env.get)}), median {med:.4f}, "
          f"left out {left_out}, emulated max|dlogit| {dl:.3e}")
    assert len(left_out) <= R.OVER_CAP[case], left_out
    assert len(tol) + len(left_out) == 49 and all(0 < t <= R.CAP for t in tol.values())
    assert 0 < dl < 5e-3
    R.gate(R.oracle_bf16_operands(*case)["grads"], r64["grads"], tol, what=str(case))
    assert R.cosine(R.oracle_bf16_operands(*case)["grads"], r64["grads"]) >= 0.999


def _fails(ours, ref, tol):
    try:
        R.gate(ours, ref, tol)
    except AssertionError as e:
        assert all(k in str(e) for k in ours)  # the failing tensor is named
        return True
    return False


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_gate_negative_controls(case):
    """One gated tensor at a time, changed in the fp64 gradients themselves: scaled by 0.7 (ratio 0.3, over
    the 0.25 cap), negated (ratio 2), the row holding its largest entry zeroed (ratio 1), and its first row
    zeroed. The first three must fail the bf16 gate and the fp32 gate for every gated tensor. A max-norm
    gate sees a dropped first row only by that row's size: it must fail the fp32 gate unless the row's true
    gradient is exactly zero (rows 0-23 of the last TA layer's conv1: end_conv reads the last 6 frames
    only), and the bf16 gate whenever the row exceeds the tensor's bound; below the bound the gate must
    report the row's size exactly. Since the gate is per tensor, the unchanged tensors (ratio 0, checked
    once on the whole set) are left out of the changed sets."""
    r64, env, tol, left_out, _ = R.bf16_reference(*case)
    g64 = r64["grads"]
    rat = R.gate(g64, g64, tol)
    assert all(v == 0.0 for v in rat.values())
    R.gate(g64, g64, R.FP32_GRAD_TOL)
    unseen = []
    for k, t in tol.items():
        g = g64[k]
        top = int(np.unravel_index(np.abs(g).argmax(), g.shape)[0])
        row_top, row0 = g.copy(), g.copy()
        row_top[top] = 0
        row0[0] = 0
        for name, changed in (("x0.7", 0.7 * g), ("negated", -g), ("largest row zeroed", row_top)):
            assert _fails({k: changed}, {k: g}, {k: t}), (k, name, "passes the bf16 gate")
            assert _fails({k: changed}, {k: g}, R.FP32_GRAD_TOL), (k, name, "passes the fp32 gate")
        size = float(np.abs(g[0]).max() / np.abs(g).max())
        assert _fails({k: row0}, {k: g}, R.FP32_GRAD_TOL) == (size > R.FP32_GRAD_TOL), (k, size)
        if size <= R.FP32_GRAD_TOL:
            assert size == 0.0 and k.endswith(("trans_layers.1.conv1.weight", "trans_layers.1.conv1.bias")), k
        assert _fails({k: row0}, {k: g}, {k: t}) == (size > t), (k, size, t)
        assert R.ratios({k: row0}, {k: g})[k] == pytest.approx(size, rel=1e-12, abs=0)
        if 0 < size <= t:
            unseen.append((k, round(size, 4), round(t, 4)))
    print(f"{case}: {len(tol)} gated tensors; first row below the bf16 bound (not visible to a max-norm gate): {unseen}")
    with pytest.raises(AssertionError):
        R.gate({k: np.full_like(v, np.nan) for k, v in g64.items()}, g64, tol)
