"""What tests/test_class_weight.py (CPU) and tests/test_gpu_class_weight.py (MI355X) share: the cases of
the class-weighted loss, the fp64 yardstick (torch.nn.functional.cross_entropy and its autograd gradient on
the CPU), the two gates, and an fp32 numpy emulation of f3_soft_ce_w's sums. Not a test module.

The gates are tests/test_gpu_accum_smoothing.py's LOSS_TOL and DOUT_TOL carrying the weight scale. With
a_nc the weighted smoothed label, m_n = sum_c a_nc (0 for an ignored row) and D the divisor (N for soft
labels, W = sum of the live rows' w[t_n] for index labels):
    |d loss|                 <= atol * max(1, sum_n m_n / D) + rtol * |want|
    |d dout| * D / max(1, m_n) <= DOUT_TOL
"""
import numpy as np
import torch

LOSS_TOL = dict(rtol=1e-5, atol=2e-5)
DOUT_TOL = 2e-6

CLASSES = (1, 2, 11, 16, 17, 64)       # both ends of the register path, the first memory-path C, the maximum
BATCHES = (1, 63, 64, 65, 257, 4096, 4097)  # one thread, a wave and its neighbours, two passes, both sides of 4096
FORMS = ("soft", "soft075", "index", "index_ignore")
SMOOTHINGS = (0.0, 0.1, 1.0)


def make_weights(rng, C):
    """2^U(-2,2) per class; with more than two classes the last one gets weight 0."""
    w = np.exp2(rng.uniform(-2.0, 2.0, C)).astype(np.float32)
    if C > 2:
        w[C - 1] = 0.0
    return w


def make_case(N, C, form, eps):
    """(out f32[N,C], label f32[N,C] or i64[N], w f32[C]), seeded by the case. Index labels: row 0 has
    class 0, whose weight is never the zero one, so W > 0; `index_ignore` sets every third row (n % 3 == 2)
    to -100."""
    rng = np.random.default_rng([N, C, FORMS.index(form), int(round(10 * eps))])
    out = rng.uniform(-4.0, 4.0, (N, C)).astype(np.float32)
    w = make_weights(rng, C)
    if form.startswith("index"):
        label = rng.integers(0, C, N).astype(np.int64)
        label[0] = 0
        if form == "index_ignore":
            label[2::3] = -100
        return out, label, w
    label = rng.random((N, C)).astype(np.float32)
    label /= label.sum(1, keepdims=True)
    if form == "soft075":  # rows that do not sum to 1: nothing renormalises them
        label = (label * np.float32(0.75)).astype(np.float32)
    return out, label, w


def live_rows(label, C):
    return (label >= 0) & (label < C)


def torch_reference(out, label, w, eps):
    """(loss, dout [N,C]) of torch.nn.functional.cross_entropy(weight=, label_smoothing=) in fp64 on the CPU;
    an index outside [0, C) becomes ignore_index (-100)."""
    C = out.shape[1]
    if label.ndim == 1:
        t = torch.from_numpy(np.where(live_rows(label, C), label, -100).astype(np.int64))
    else:
        t = torch.from_numpy(label.astype(np.float64))
    with torch.enable_grad():  # (also when the caller runs under no_grad)
        o = torch.from_numpy(out.astype(np.float64)).requires_grad_(True)
        loss = torch.nn.functional.cross_entropy(o, t, weight=torch.from_numpy(w.astype(np.float64)),
                                                 label_smoothing=float(eps))
        (g,) = torch.autograd.grad(loss, o)
    return float(loss.item()), g.numpy()


def scales(label, w, eps, C):
    """(m_n per row, D) in fp64."""
    w64 = w.astype(np.float64)
    N = label.shape[0]
    if label.ndim == 1:
        live = live_rows(label, C)
        y = np.zeros((N, C))
        y[np.flatnonzero(live), label[live]] = 1.0
        a = (y * (1.0 - eps) + eps / C) * w64 * live[:, None]
        D = float(w64[label[live]].sum())
    else:
        a = (label.astype(np.float64) * (1.0 - eps) + eps / C) * w64
        D = float(N)
    return a.sum(1), D


def gate_ratios(loss, dout, out, label, w, eps, want=None):
    """(loss gate used, dout gate used), each as a fraction of its bound (<= 1 passes)."""
    want_l, want_d = torch_reference(out, label, w, eps) if want is None else want
    m, D = scales(label, w, eps, out.shape[1])
    bound = LOSS_TOL["atol"] * max(1.0, m.sum() / D) + LOSS_TOL["rtol"] * abs(want_l)
    rl = abs(float(loss) - want_l) / bound
    rd = 0.0
    if dout is not None:
        err = np.abs(dout.astype(np.float64) - want_d) * D / np.maximum(1.0, m)[:, None]
        rd = float(err.max()) / DOUT_TOL
    return rl, rd


# ---- the kernel's sums in fp32 ---------------------------------------------------------------------
def _block_sum(v):
    """sce_block_sum over 256 fp32 thread values: xor-shuffles inside each wave, then the four wave sums."""
    v = v.astype(np.float32).reshape(4, 64).copy()
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, lane ^ off]).astype(np.float32)
    r = v[:, 0]
    return np.float32(np.float32(np.float32(r[0] + r[1]) + r[2]) + r[3])


def emulate(out, label, w, eps):
    """f3_soft_ce_w in numpy: fp32 throughout, every sum sequential in the kernel's order, products rounded
    before they are added (the kernel fuses them: one rounding fewer), W summed in fp64 and rounded to
    fp32 once. Returns (loss f32, dout f32[N,C])."""
    f = np.float32
    N, C = out.shape
    keep, share = f(f(1.0) - f(eps)), f(f(eps) / f(C))
    if label.ndim == 1:
        live = live_rows(label, C)
        y = np.zeros((N, C), dtype=f)
        y[np.flatnonzero(live), label[live]] = 1.0
        D = f(w.astype(np.float64)[label[live]].sum())
    else:
        live = np.ones(N, dtype=bool)
        y = label.astype(f)
        D = f(N)
    a = ((y * keep + share).astype(f) * w[None, :]).astype(f)
    mx = out.max(1)
    s = np.zeros(N, dtype=f)
    m = np.zeros(N, dtype=f)
    for c in range(C):
        s = (s + np.exp((out[:, c] - mx).astype(f)).astype(f)).astype(f)
        m = (m + a[:, c]).astype(f)
    lse = (mx + np.log(s).astype(f)).astype(f)
    l = np.zeros(N, dtype=f)
    dout = np.zeros((N, C), dtype=f)
    with np.errstate(divide="ignore", invalid="ignore"):
        for c in range(C):
            z = (out[:, c] - lse).astype(f)
            l = (l - (a[:, c] * z).astype(f)).astype(f)
            v = ((np.exp(z).astype(f) * m).astype(f) - a[:, c]).astype(f)
            dout[:, c] = (np.where(live, v, f(0.0)) / D).astype(f)
        l = np.where(live, l, f(0.0)).astype(f)
        one = N <= 4096
        grid = 1 if one else min((N + 255) // 256, 1024)
        parts = []
        for b in range(grid):
            lsum = np.zeros(256, dtype=f)
            for start in range(b * 256, N, grid * 256):
                rows = l[start:start + 256]
                lsum[:rows.size] = (lsum[:rows.size] + rows).astype(f)
            parts.append(_block_sum(lsum))
        total = f(0.0)
        if one:
            total = parts[0]
        else:
            for p in parts:
                total = f(total + p)
        return f(total / D), dout
