"""The bf16x3 step's gcn forward with the graph mix fused into the 1x1 GEMM (gcn_fwd.hip, f3_gcn_fwd_mix_x3):
Z = A~ x (bf16x3), split into [z_hi | z_lo] rows, g = Z W + bias_v (bf16x3) with the BN1 sums, Z written once and
never read back. Needs an MI355X.

The kernel is pw_gemm's with the A blocks computed instead of loaded, so everything is compared bit for bit with
the pair it replaces (f3_graph_mix_forward_ex(F3_MIX_X3 | F3_MIX_Z3) then f3_conv_step_x3cat(F3_STEP_GCN_FWD)); the
fp64 gate is the project's bf16x3 tolerance, 1e-4 of max|ref| (tests/test_gpu_parity.py X3_TOL)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X3_TOL = 1e-4

# (V, K, Cin, C, F): ragged last tile with frames straddling tiles; WN = 2; a single partial tile; the 14-joint
# layout; odd V; 788 tiles (the last half full): per workgroup several tiles, range boundaries inside frames
BIG = (18, 3, 64, 64, 1400)
CASES = [(18, 3, 64, 64, 19), (18, 3, 64, 128, 19), (18, 3, 64, 64, 1), (14, 3, 64, 64, 23), (17, 3, 64, 128, 7), BIG]
_ids = lambda c: "-".join(map(str, c))


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda")


@functools.lru_cache(maxsize=None)
def _case(V, K, Cin, C, F):
    """Inputs (fp32, on the CPU) and the fp64 reference of one case; computed once, never modified."""
    gen = torch.Generator().manual_seed(V * 13 + K * 7 + Cin + 3 * C + F)
    A = (torch.rand(K, V, V, dtype=torch.float64, generator=gen) / V).float()
    x = torch.randn(F, V, Cin, generator=gen)
    W = (torch.randn(C, K * Cin, generator=gen) / np.sqrt(K * Cin)).float()
    bv = 0.1 * torch.randn(V, C, generator=gen)
    z = torch.einsum("kvw,fvc->fwkc", A.double(), x.double()).reshape(F * V, K * Cin)
    g = z @ W.double().t() + bv.double().repeat(F, 1)
    return A, x, W, bv, z, g, g.sum(0), (g * g).sum(0)


def _bufs(case, d):
    V, K, Cin, C, F = case
    z3 = torch.full((F * V, 2 * K * Cin), float("nan"), device=d, dtype=torch.bfloat16)
    g = torch.full((F * V, C), float("nan"), device=d)
    return z3, g, torch.zeros(C, device=d, dtype=torch.float64), torch.zeros(C, device=d, dtype=torch.float64)


def _inputs(case, d):
    V, K, Cin, C, F = case
    A, x, W, bv = _case(*case)[:4]
    return (A.contiguous().to(d), x.contiguous().to(d), W.contiguous().to(d), bv.contiguous().to(d),
            torch.empty(C * K * Cin + 64, device=d))


def _fused(case, d):
    import fall_multimodal_amd._lib as L
    V, K, Cin, C, F = case
    Ag, xg, Wg, bg, wp = _inputs(case, d)
    z3, g, ss, sq = _bufs(case, d)
    L.check(L.lib().f3_gcn_fwd_mix_x3(L.ptr(Ag), L.ptr(xg), L.ptr(Wg), L.ptr(wp), L.ptr(bg), L.ptr(z3), L.ptr(g),
                                      L.ptr(ss), L.ptr(sq), F, K, V, Cin, C, L.stream_handle()), "gcn_fwd_mix")
    torch.cuda.synchronize()
    return z3, g, ss, sq


def _pair(case, d):
    """The two kernels the fused one replaces: the mix into [z_hi | z_lo] rows, then the gcn GEMM over them."""
    import fall_multimodal_amd._lib as L
    V, K, Cin, C, F = case
    Ag, xg, Wg, bg, wp = _inputs(case, d)
    z3, g, ss, sq = _bufs(case, d)
    lib, st = L.lib(), L.stream_handle()
    L.check(lib.f3_graph_mix_forward_ex(L.ptr(Ag), L.ptr(xg), L.ptr(z3), F, K, V, Cin, 4 | 8, st), "mix z3")
    L.check(lib.f3_conv_step_x3cat(0, L.ptr(z3), L.ptr(Wg), L.ptr(wp), L.ptr(g), L.ptr(bg), None, None, None, None,
                                   None, 0.0, L.ptr(ss), L.ptr(sq), 1, F, V, K * Cin, C, st), "gcn fwd")
    torch.cuda.synchronize()
    return z3, g, ss, sq


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_same_bits_as_the_pair(case):
    """Z rows, g and the fp64 BN1 sums (the same fp32 partials, which fp64 adds exactly in any order)."""
    d = dev()
    z3, g, ss, sq = _fused(case, d)
    pz3, pg, pss, psq = _pair(case, d)
    assert torch.equal(z3.view(torch.int16), pz3.view(torch.int16))
    assert torch.equal(g, pg), float((g - pg).abs().max())
    assert torch.equal(ss, pss) and torch.equal(sq, psq)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_fused_matches_fp64(case):
    d = dev()
    V, K, Cin, C, F = case
    rz, rg, rs, rq = _case(*case)[4:]
    z3, g, ss, sq = _fused(case, d)
    zs = z3[:, :K * Cin].double().cpu() + z3[:, K * Cin:].double().cpu()
    ez = float((zs - rz).abs().max() / rz.abs().max())
    eg = float((g.double().cpu() - rg).abs().max() / rg.abs().max())
    # the sums relative to the largest column sum, as every gate here is of max|ref| (a column sum is a random
    # walk around zero; one that happens to come out 1e-2 of the typical size carries the same absolute error)
    es = float((ss.cpu() - rs).abs().max() / rs.abs().max())
    eq = float((sq.cpu() - rq).abs().max() / rq.abs().max())
    print(f"gcn fwd+mix fused V,K,Cin,C,F={case}: Z {ez:.2e}, g {eg:.2e} of max|ref|; sum {es:.2e}, sumsq {eq:.2e} rel")
    assert torch.isfinite(g).all()
    assert ez <= X3_TOL and eg <= X3_TOL, (ez, eg)
    assert es <= 1e-4 and eq <= 1e-4, (es, eq)


def test_run_to_run_identical():
    d = dev()
    a, b = _fused(BIG, d), _fused(BIG, d)
    assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16))
    for u, v in zip(a[1:], b[1:]):
        assert torch.equal(u, v)


@pytest.mark.parametrize("V,K,Cin,C", [(18, 3, 128, 128), (18, 1, 64, 64), (22, 3, 64, 64), (18, 3, 64, 256)],
                         ids=["Cin128", "K1", "V22", "C256"])
def test_refusals(V, K, Cin, C):
    d = dev()
    import fall_multimodal_amd._lib as L
    F = 2
    buf = lambda *s: torch.zeros(*s, device=d)
    z3 = torch.full((F * V, 2 * K * Cin), 7.0, device=d, dtype=torch.bfloat16)
    g = torch.full((F * V, C), 7.0, device=d)
    ss, sq = torch.zeros(C, device=d, dtype=torch.float64), torch.zeros(C, device=d, dtype=torch.float64)
    st = L.lib().f3_gcn_fwd_mix_x3(L.ptr(buf(K, V, V)), L.ptr(buf(F, V, Cin)), None, L.ptr(buf(C * K * Cin + 64)),
                                   L.ptr(buf(V, C)), L.ptr(z3), L.ptr(g), L.ptr(ss), L.ptr(sq), F, K, V, Cin, C,
                                   L.stream_handle())
    torch.cuda.synchronize()
    assert st == L.F3_EINVAL
    assert bool((z3 == 7.0).all()) and bool((g == 7.0).all()) and not ss.any() and not sq.any()


def _step_dump(out_path):
    """One TrainStep of the B = 4 3-stream bf16x3 model; run in a child process (the switch is read once)."""
    sys.path.insert(0, ROOT)
    import fall_multimodal_amd as f3
    from oracle import model_cpu as oc
    from oracle.prng import synthetic_batch
    d = torch.device("cuda")
    spec = oc.Spec(model="two_stgcan_bilstm", layout="coco_mmpose", num_class=11, sensor_dim=6)
    model = f3.TwoStreamSTGCAN_BiLSTM(3, {"layout": "coco_mmpose", "strategy": "spatial"}, 11, 6, device=d,
                                      precision="bf16x3")
    model.load_state_dict(oc.init_state(spec, 21))
    B = 4
    step = f3.TrainStep(model, B, lr=1e-3)
    sk, se, lb = (torch.from_numpy(x).to(d) for x in synthetic_batch(B, 18, 11, 6, 8))
    loss = step(sk, se, lb)
    torch.cuda.synchronize()
    np.savez(out_path, loss=loss.cpu().numpy(), logits=step.out.cpu().numpy(), grads=step.grads.cpu().numpy(),
             params=model.flat_parameters().detach().cpu().numpy())


def test_step_bits_do_not_depend_on_the_switch(tmp_path):
    """Loss, logits, flat gradient and updated parameters of one step, F3_GCN_FWD_FUSED=0 against the default."""
    dev()
    outs = []
    for name, val in (("pair", "0"), ("fused", None)):
        out = tmp_path / f"{name}.npz"
        env = {k: v for k, v in os.environ.items() if k != "F3_GCN_FWD_FUSED"}
        if val is not None:
            env["F3_GCN_FWD_FUSED"] = val
        code = (f"import sys; sys.path.insert(0, {ROOT!r}); import tests.test_gpu_gcn_fwd_mix as t; "
                f"t._step_dump({str(out)!r})")
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append(np.load(out))
    for k in ("loss", "logits", "grads", "params"):
        a, b = outs[0][k], outs[1][k]
        assert np.isfinite(b).all(), k
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (k, float(np.abs(a - b).max()))
