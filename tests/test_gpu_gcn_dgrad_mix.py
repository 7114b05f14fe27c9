"""The bf16x3 step's fused gcn input gradient + graph-mix backward (gcn_bwd.hip, f3_gcn_dgrad_mix_x3):
dZ = dg W (bf16x3), split again, then dx = A~ dZ and dA = x dZ (bf16x3), dZ never in HBM. Needs an MI355X.

Gate: the project's bf16x3 tolerance, 1e-4 of max|ref| against fp64 on the fp32 operands
(tests/test_gpu_parity.py X3_TOL). A CPU emulation of the whole split chain gives 5.4e-6 .. 7.6e-6 of
max|ref| for dx and dA on these shapes and generators, so the gate has ~13x headroom."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

X3_TOL = 1e-4

# (V, K, Cin, C, F): ragged frame counts, both joint layouts and an odd V, K = 1, every (Cin, C) of the step
CASES = [(18, 3, 64, 64, 19), (18, 3, 64, 128, 19), (18, 3, 128, 128, 8), (14, 3, 128, 256, 11),
         (18, 3, 256, 256, 9), (17, 1, 64, 64, 5), (18, 3, 64, 64, 1)]
LOOP_CASES = [(18, 3, 64, 64, 37), (18, 3, 128, 256, 21)]


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda")


@functools.lru_cache(maxsize=None)
def _case(V, K, Cin, C, F):
    """Inputs (fp32, on the CPU) and the fp64 reference of one case; computed once, never modified."""
    g = torch.Generator().manual_seed(V * 13 + K * 7 + Cin + 3 * C + F)
    A = (torch.rand(K, V, V, dtype=torch.float64, generator=g) / V).float()
    x = torch.randn(F, V, Cin, generator=g)
    dg = torch.randn(F, V, C, generator=g)
    W = torch.randn(C, K * Cin, generator=g) / np.sqrt(K * Cin)
    dz = (dg.double().reshape(F * V, C) @ W.double()).reshape(F, V, K, Cin)  # [f][w][k][ci]
    dx = torch.einsum("kvw,fwkc->fvc", A.double(), dz)
    dA = torch.einsum("fvc,fwkc->kvw", x.double(), dz)
    return A, x, dg, W, dx, dA


def _split(lib, L, t, d):
    t = t.float().contiguous().to(d)
    out = torch.empty(t.numel() // t.shape[-1], 2 * t.shape[-1], device=d, dtype=torch.bfloat16)
    L.check(lib.f3_split_x3cat(L.ptr(t), L.ptr(out), t.numel() // t.shape[-1], t.shape[-1], L.stream_handle()), "split")
    return out


def _fused(case, d, accumulate=0, max_wg=0, dx0=None):
    import fall_multimodal_amd._lib as L
    V, K, Cin, C, F = case
    A, x, dg, W, _, _ = _case(*case)
    lib, st = L.lib(), L.stream_handle()
    dg3 = _split(lib, L, dg, d)
    Ag, xg, Wg = A.contiguous().to(d), x.contiguous().to(d), W.contiguous().to(d)
    wp = torch.empty(C * K * Cin + 64, device=d)
    dx = dx0.clone() if dx0 is not None else torch.full((F, V, Cin), float("nan"), device=d)
    dA = torch.full((K, V, V), float("nan"), device=d)
    L.check(lib.f3_gcn_dgrad_mix_x3(L.ptr(dg3), L.ptr(Wg), L.ptr(wp), L.ptr(Ag), L.ptr(xg), L.ptr(dx), L.ptr(dA), F, K,
                                    V, Cin, C, accumulate, max_wg, st), "gcn_dgrad_mix")
    torch.cuda.synchronize()
    return dx, dA


def _pair(case, d):
    """The two kernels the fused one replaces: the gcn input-gradient GEMM into fp32 dZ, then the mix backward."""
    import fall_multimodal_amd._lib as L
    V, K, Cin, C, F = case
    A, x, dg, W, _, _ = _case(*case)
    lib, st = L.lib(), L.stream_handle()
    dg3 = _split(lib, L, dg, d)
    Ag, xg, Wg = A.contiguous().to(d), x.contiguous().to(d), W.contiguous().to(d)
    wp = torch.empty(C * K * Cin + 64, device=d)
    dz = torch.empty(F, V, K * Cin, device=d)
    L.check(lib.f3_conv_backward_data_x3cat(L.ptr(dg3), L.ptr(Wg), L.ptr(dz), L.ptr(wp), 1, F, V, K * Cin, C, 1, 1, 0,
                                            st), "dgrad")
    dx = torch.empty(F, V, Cin, device=d)
    dA = torch.empty(K, V, V, device=d)
    L.check(lib.f3_graph_mix_backward_ex(L.ptr(Ag), L.ptr(xg), L.ptr(dz), L.ptr(dx), L.ptr(dA), F, K, V, Cin, 4, st),
            "mixbwd")
    torch.cuda.synchronize()
    return dx, dA


def _errs(case, dx, dA):
    _, _, _, _, rdx, rdA = _case(*case)
    out = {}
    for name, got, ref in (("dx", dx, rdx), ("dA", dA, rdA)):
        r = ref.numpy()
        out[name] = float(np.abs(got.cpu().double().numpy() - r).max() / np.abs(r).max())
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_fused_matches_fp64(case):
    d = dev()
    dx, dA = _fused(case, d)
    e = _errs(case, dx, dA)
    print(f"gcn dgrad+mix fused V,K,Cin,C,F={case}: dx {e['dx']:.2e}, dA {e['dA']:.2e} of max|ref|")
    assert torch.isfinite(dx).all() and torch.isfinite(dA).all()
    assert e["dx"] <= X3_TOL and e["dA"] <= X3_TOL, e


@pytest.mark.parametrize("case", [(18, 3, 64, 64, 19), (18, 3, 256, 256, 9)], ids=lambda c: "-".join(map(str, c)))
def test_accumulate_is_prefill_plus_result(case):
    """accumulate=1 adds the same sums to the pre-filled dx with one fp32 add per element: bit for bit."""
    d = dev()
    V, K, Cin, C, F = case
    dx, dA = _fused(case, d)
    pre = torch.randn(F, V, Cin, generator=torch.Generator().manual_seed(5)).to(d)
    dx1, dA1 = _fused(case, d, accumulate=1, dx0=pre)
    assert torch.equal(dx1, pre + dx), float((dx1 - (pre + dx)).abs().max())
    assert torch.equal(dA1, dA)


@pytest.mark.parametrize("case", LOOP_CASES, ids=lambda c: "-".join(map(str, c)))
def test_persistent_loop(case):
    """Few workgroups: each walks several frames, the last round only partly filled."""
    d = dev()
    nch = case[2] // 64
    for wgs in (nch, 2 * nch):
        dx, dA = _fused(case, d, max_wg=wgs)
        e = _errs(case, dx, dA)
        print(f"gcn dgrad+mix fused V,K,Cin,C,F={case} workgroups={wgs}: dx {e['dx']:.2e}, dA {e['dA']:.2e}")
        assert e["dx"] <= X3_TOL and e["dA"] <= X3_TOL, (wgs, e)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_fused_against_the_pair(case):
    """Same three split products and the same dZ split as the GEMM + mix pair: only fp32 summation order
    differs, so the fused error stays within 2x the pair's + 1e-6 of max|ref|."""
    d = dev()
    ef = _errs(case, *_fused(case, d))
    ep = _errs(case, *_pair(case, d))
    print(f"gcn dgrad+mix V,K,Cin,C,F={case}: fused dx {ef['dx']:.2e} dA {ef['dA']:.2e}; "
          f"pair dx {ep['dx']:.2e} dA {ep['dA']:.2e}")
    for k in ("dx", "dA"):
        assert ef[k] <= X3_TOL and ep[k] <= X3_TOL, (k, ef, ep)
        assert ef[k] <= 2 * ep[k] + 1e-6, (k, ef, ep)


@pytest.mark.parametrize("case", [c for c in CASES + LOOP_CASES if c[3] <= 128], ids=lambda c: "-".join(map(str, c)))
def test_same_bits_as_the_pair(case):
    """What the step relies on where it dispatches the fused kernel (Cin = 64): the same MFMA chain per dZ
    element as the GEMM (C <= 128: one wave sums all of C), so dx is the pair's bit for bit; and with one
    channel chunk and the mix backward's workgroup count (here one per frame) the same frames per partial
    row, so dA is too."""
    d = dev()
    V, K, Cin, C, F = case
    dx, dA = _fused(case, d, max_wg=min(F, 768) * (Cin // 64))
    pdx, pdA = _pair(case, d)
    assert torch.equal(dx, pdx), float((dx - pdx).abs().max())
    if Cin == 64:
        assert torch.equal(dA, pdA), float((dA - pdA).abs().max())


@pytest.mark.parametrize("case", [(18, 3, 64, 128, 19), (18, 3, 256, 256, 9)], ids=lambda c: "-".join(map(str, c)))
def test_run_to_run_identical(case):
    d = dev()
    dx0, dA0 = _fused(case, d)
    dx1, dA1 = _fused(case, d)
    assert torch.equal(dx0, dx1) and torch.equal(dA0, dA1)


@pytest.mark.parametrize("V,K,Cin,C", [(18, 3, 96, 128), (33, 1, 64, 64), (22, 3, 64, 64)],
                         ids=["Cin96", "V33", "KV66"])
def test_refusals(V, K, Cin, C):
    d = dev()
    import fall_multimodal_amd._lib as L
    F = 2
    buf = lambda *s: torch.zeros(*s, device=d)
    dg3 = torch.zeros(F * V, 2 * C, device=d, dtype=torch.bfloat16)
    st = L.lib().f3_gcn_dgrad_mix_x3(L.ptr(dg3), None, L.ptr(buf(C * K * Cin + 64)), L.ptr(buf(K, V, V)),
                                     L.ptr(buf(F, V, Cin)), L.ptr(buf(F, V, Cin)), L.ptr(buf(K, V, V)), F, K, V, Cin, C,
                                     0, 0, L.stream_handle())
    assert st == L.F3_EINVAL
