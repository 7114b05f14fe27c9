"""Optimizers with the reference's semantics on the fused HIP kernels.

Reference: build_optimizer(model, config) -> (optimizer, scheduler) with OPTIM.TYPE in
rmsprop / sgd / adam / adamw (Multimodal_Fall3/model/optimizer.py:8-35). All four branches are
native: f3.RMSprop, f3.SGD, f3.Adam and f3.AdamW are torch.optim.Optimizer subclasses with torch's
constructor arguments, torch's arithmetic and torch's state_dict layout (state keys `square_avg`;
`momentum_buffer`; `step`, `exp_avg`, `exp_avg_sq`), so a checkpoint written by either
implementation loads into the other. The update is one fall3::rmsprop_ / fall3::optim_ launch over
the flat parameter range (f3_rmsprop_step / f3_optim_step). TrainStep(optimizer=...) takes the kind and
the hyper-parameters from such an optimizer and runs the update inside the fused step
(train.py); the conversions between its flat state buffers and the torch state_dict layout are the
pure functions flat_to_state_dict / state_dict_to_flat below.

Not built (NotImplementedError): SGD dampening, amsgrad, maximize, centered RMSprop, RMSprop momentum.
"""
from __future__ import annotations

import math

import torch

from . import ops  # noqa: F401  (registers fall3::rmsprop_ / fall3::optim_)
from ._lib import OPT_ADAM, OPT_ADAMW, OPT_RMSPROP, OPT_SGD, require_device

KIND_IDS = {"rmsprop": OPT_RMSPROP, "sgd": OPT_SGD, "adam": OPT_ADAM, "adamw": OPT_ADAMW}
_TORCH_CLASS = {"rmsprop": torch.optim.RMSprop, "sgd": torch.optim.SGD, "adam": torch.optim.Adam,
                "adamw": torch.optim.AdamW}


def _flat_view(t, start, n):
    """1-D view of n elements of t's storage from element `start`."""
    return torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage(), start, (n,))


def optimizer_kind(opt):
    """"rmsprop" / "sgd" / "adam" / "adamw" from an optimizer's class (the native classes or torch's)."""
    if isinstance(opt, (AdamW, torch.optim.AdamW)):  # torch's AdamW subclasses Adam
        return "adamw"
    if isinstance(opt, (Adam, torch.optim.Adam)):
        return "adamw" if opt.param_groups[0].get("decoupled_weight_decay") else "adam"
    if isinstance(opt, (SGD, torch.optim.SGD)):
        return "sgd"
    return "rmsprop"  # RMSprop, or any object whose param_groups[0] carries lr / alpha / eps


def check_supported(kind, group):
    """The settings the native updates do not build raise, as the configuration guards elsewhere do."""
    bad = []
    if group.get("maximize"):
        bad.append("maximize")
    if kind == "sgd" and group.get("dampening", 0) != 0:
        bad.append("dampening")
    if kind in ("adam", "adamw") and group.get("amsgrad"):
        bad.append("amsgrad")
    if kind == "rmsprop" and group.get("centered"):
        bad.append("centered")
    if kind == "rmsprop" and group.get("momentum", 0) != 0:
        bad.append("RMSprop momentum")
    if bad:
        raise NotImplementedError(f"fall3 {kind}: {', '.join(bad)} not built (see optim.py)")
    if kind == "sgd" and group.get("nesterov") and group.get("momentum", 0) <= 0:
        raise ValueError("Nesterov momentum requires a momentum and zero dampening")


def state_keys(kind, group):
    """torch's per-parameter state tensors of a kind, in the order (state0, state1) of f3_optim_step."""
    if kind == "rmsprop":
        return ("square_avg",)
    if kind == "sgd":
        return ("momentum_buffer",) if group.get("momentum", 0) != 0 else ()
    return ("exp_avg", "exp_avg_sq")


def hyper(kind, group):
    """The fall3::optim_ / f3_optim_config hyper-parameters of a param_group (absent keys: torch's defaults)."""
    b = group.get("betas", (0.9, 0.999))
    return dict(kind=KIND_IDS[kind], nesterov=bool(group.get("nesterov", False)), lr=float(group["lr"]),
                alpha=float(group.get("alpha", 0.99)), eps=float(group.get("eps", 1e-8)),
                momentum=float(group.get("momentum", 0.0)) if kind == "sgd" else 0.0, beta1=float(b[0]),
                beta2=float(b[1]), weight_decay=float(group.get("weight_decay", 0.0)))


STRUCTURE_FIELDS = ("the optimizer kind", "nesterov", "momentum zero / nonzero",
                    "plain RMSprop (no weight decay, no clipping) or not", "max_norm off / on")


def hyper_structure(kind, group, max_norm):
    """What a recorded optimizer graph fixes: which launches the step has and which kernel variant they
    run, (kind, nesterov, momentum != 0, legacy, max_norm > 0) in STRUCTURE_FIELDS order. legacy is plain
    RMSprop, f3_rmsprop_step's kernel. Everything else of a param_group and of max_norm is a value: the
    device block of f3_optim_hyper_set carries it and a replayed graph follows it."""
    h = hyper(kind, group)
    clip = bool(max_norm) and max_norm > 0
    legacy = kind == "rmsprop" and h["weight_decay"] == 0 and not max_norm
    return (kind, h["nesterov"] if kind == "sgd" else False, h["momentum"] != 0, legacy, clip)


def torch_defaults(kind, **over):
    """A complete param_group (without 'params') as torch.optim.<kind> builds it, so a state_dict's
    param_groups carries every key torch's own would."""
    d = dict(_TORCH_CLASS[kind]([torch.nn.Parameter(torch.zeros(1))], lr=1e-3).defaults)
    d.update(over)
    return d


# ---------------------------------------------------------------------------------------------
# flat state buffers <-> torch state_dict (pure; CPU or device tensors)
# ---------------------------------------------------------------------------------------------
def flat_to_state_dict(kind, group, layout, buffers, step):
    """torch.optim.<kind>(model.parameters()).state_dict() from flat state buffers.
    layout: [(shape, offset, nograd)] in model.parameters() order (offsets into the flat buffers);
    buffers: the flat state tensors in state_keys order; step: optimizer steps taken; group: the
    param_group without 'params'. No-gradient entries carry no state, and before the first step the
    state is empty, as in torch."""
    keys = state_keys(kind, group)
    if len(buffers) != len(keys):
        raise ValueError(f"{kind}: expected {len(keys)} state buffers, got {len(buffers)}")
    state = {}
    if step > 0:
        for i, (shape, off, nograd) in enumerate(layout):
            if nograd:
                continue
            n = int(math.prod(shape))
            st = {}
            if kind != "sgd":
                st["step"] = torch.tensor(float(step), dtype=torch.float32)
            for k, buf in zip(keys, buffers):
                st[k] = buf[off:off + n].detach().clone().view(shape)
            if st:
                state[i] = st
    g = {k: v for k, v in group.items() if k != "params"}
    g["params"] = list(range(len(layout)))
    return {"state": state, "param_groups": [g]}


def state_dict_to_flat(kind, sd, layout, nparam, device="cpu"):
    """The inverse: (flat state buffers in state_keys order (pads and no-gradient entries zero), step,
    the saved param_group). Every parameter with state must agree on `step`."""
    groups = sd["param_groups"]
    if len(groups) != 1 or len(groups[0]["params"]) != len(layout):
        raise ValueError("optimizer state_dict: one param_group over every model parameter expected")
    group = groups[0]
    keys = state_keys(kind, group)
    buffers = [torch.zeros(nparam, dtype=torch.float32, device=device) for _ in keys]
    steps = set()
    for idx, i in zip(group["params"], range(len(layout))):
        st = sd["state"].get(idx)
        if not st:
            continue
        shape, off, nograd = layout[i]
        if nograd:
            raise ValueError(f"optimizer state_dict: state for parameter {i}, which never receives a gradient")
        n = int(math.prod(shape))
        if "step" in st:
            steps.add(int(st["step"]))
        for k, buf in zip(keys, buffers):
            if k not in st:
                raise ValueError(f"optimizer state_dict: parameter {i} has no '{k}' (saved by another optimizer?)")
            if tuple(st[k].shape) != tuple(shape):
                raise ValueError(f"optimizer state_dict: '{k}' of parameter {i} has shape {tuple(st[k].shape)}")
            buf[off:off + n].copy_(st[k].reshape(-1).to(dtype=torch.float32))
    if len(steps) > 1:
        raise ValueError(f"optimizer state_dict: parameters disagree on step ({sorted(steps)})")
    step = steps.pop() if steps else (1 if sd["state"] else 0)  # SGD keeps no count: "has stepped"
    return buffers, step, group


class _FlatOptimizer(torch.optim.Optimizer):
    """Flat path shared by the native optimizers: the fall3 modules keep their parameters as views of
    ONE flat buffer and loss.backward() hands back their gradients as views of ONE flat gradient buffer
    in the same layout (ops.py `_split_grads`). When a group's parameters, gradients and state tensors
    are laid out that way, step() is one launch over the whole range (the 16-B alignment pads between
    tensors carry zero parameters and zero gradients, so every update leaves them unchanged), and the
    group shares one `step` counter tensor. Anything else (a user-built group, states loaded from a
    state_dict, gradients that autograd copied, a parameter without a gradient) takes the per-tensor
    path."""

    KIND = None

    def _keys(self, group):
        return state_keys(self.KIND, group)

    def _flat(self, group):
        """(params, *states, grads) flat views covering the group, or None. The full layout check
        below is ~7 us of Python per parameter; once it has passed, the group remembers the layout
        and later steps only check that the gradients are still views of one buffer at the same
        relative offsets (the parameters and the flat states do not move between steps)."""
        ps = group["params"]
        if not ps or any(p.grad is None for p in ps):
            return None
        keys = self._keys(group)
        caches = self.__dict__.setdefault("_f3_flat", {})  # per group (not in param_groups: state_dict)
        cache = caches.get(id(group))
        if cache is not None:
            hit = self._flat_cached(ps, cache) if cache[6] == keys else None
            if hit is not None:
                return hit
            del caches[id(group)]
        self.__dict__["_f3_keys"] = keys  # the group's state keys, for _flat_full(ps)
        flat = self._flat_full(ps)
        if flat is not None:
            p0 = min(ps, key=lambda t: t.storage_offset())
            caches[id(group)] = (tuple(map(id, ps)), [p.storage_offset() - p0.storage_offset() for p in ps], flat[0],
                                 flat[1:-1], tuple(self.state[p0][k] for k in keys), p0, keys)
        return flat

    def _flat_cached(self, ps, cache):
        """The remembered layout still holds when every gradient is contiguous and sits at its
        parameter's relative offset from the first gradient, and that gradient's storage spans the
        whole range: the gradients then ARE the range of one buffer. (Addresses, not `_base`: the
        autograd engine hands parameters detached gradients, which share the buffer but are not
        views of it, so a `_base` test failed on every step and sent it to the full ~7 us/parameter
        check.)"""
        ids, rel, flat_p, flat_states, st0, p0, keys = cache
        if tuple(map(id, ps)) != ids or any(self.state[p0].get(k) is not s for k, s in zip(keys, st0)):
            return None
        g0 = p0.grad
        if g0.dtype != torch.float32 or g0.device != p0.device:
            return None
        n = flat_p.numel()
        gbase = g0.storage_offset()
        if (gbase + n) * 4 > g0.untyped_storage().nbytes():
            return None
        a0 = g0.data_ptr()
        for p, r in zip(ps, rel):
            g = p.grad
            if g is None or g.data_ptr() - a0 != 4 * r or not g.is_contiguous() or g.dtype != torch.float32:
                return None
        return (flat_p, *flat_states, _flat_view(g0, gbase, n))

    def _flat_full(self, ps):
        keys = self.__dict__.get("_f3_keys")
        keys = self._keys(self.param_groups[0]) if keys is None else keys
        ps = sorted(ps, key=lambda t: t.storage_offset())  # module order is not the flat order
        p0, g0 = ps[0], ps[0].grad
        if p0.dtype != torch.float32 or g0.dtype != torch.float32:
            return None
        pst, gst = p0.untyped_storage().data_ptr(), g0.untyped_storage().data_ptr()
        pbase, gbase = p0.storage_offset(), g0.storage_offset()
        st0 = self.state[p0]
        first = [st0.get(k) for k in keys]
        if any((s is None) != (first[0] is None) for s in first):
            return None
        fresh = bool(keys) and first[0] is None
        sst = [s.untyped_storage().data_ptr() if s is not None else None for s in first]
        sbase = [s.storage_offset() if s is not None else 0 for s in first]
        end = pbase
        for i, p in enumerate(ps):
            g = p.grad
            # every tensor starts exactly at the previous one's end rounded up to 16 B: a larger gap
            # could hold a tensor outside this group (another param_group, a frozen parameter), which
            # one launch over [first, last] would update with this group's lr
            if (p.untyped_storage().data_ptr() != pst or g.untyped_storage().data_ptr() != gst
                    or not p.is_contiguous() or not g.is_contiguous() or g.shape != p.shape
                    or (i > 0 and p.storage_offset() != (end + 3) // 4 * 4)
                    or g.storage_offset() - gbase != p.storage_offset() - pbase):
                return None
            for j, k in enumerate(keys):
                s = self.state[p].get(k)
                if (s is None) != fresh or (s is not None and (
                        s.untyped_storage().data_ptr() != sst[j]
                        or s.storage_offset() - sbase[j] != p.storage_offset() - pbase)):
                    return None
            end = p.storage_offset() + p.numel()
        n = end - pbase
        if fresh:
            # first step: one flat buffer per state key, per-tensor views as the states
            flats = [torch.zeros(n, dtype=torch.float32, device=p0.device) for _ in keys]
            step = torch.zeros((), dtype=torch.float32)
            for p in ps:
                o = p.storage_offset() - pbase
                for k, f in zip(keys, flats):
                    self.state[p][k] = f[o:o + p.numel()].view_as(p)
                if self.KIND != "sgd":
                    self.state[p]["step"] = step
        else:
            flats = [_flat_view(s, b, n) for s, b in zip(first, sbase)]
        return (_flat_view(p0, pbase, n), *flats, _flat_view(g0, gbase, n))

    # -- the update -----------------------------------------------------------------------------
    def _scalars(self, device, t):
        """The group-independent step-scalar block of this optimizer on `device`, its device step
        count set to t (the count before this step; the kernel's begin increments it)."""
        blocks = self.__dict__.setdefault("_f3_scalars", {})
        ent = blocks.get(device)
        if ent is None:
            ent = blocks[device] = [ops.optim_scalars(device), 0]
        if ent[1] != t:
            ops.scalar_views(ent[0])[0].fill_(t)
        ent[1] = t + 1
        return ent[0]

    def _update(self, group, p, states, g, t):
        h = hyper(self.KIND, group)
        none = p.new_empty(0)
        s0 = states[0] if len(states) > 0 else none
        s1 = states[1] if len(states) > 1 else p.new_empty(0)
        torch.ops.fall3.optim_(p, s0, s1, self._scalars(p.device, t), g, h["kind"], h["nesterov"], h["lr"],
                               h["alpha"], h["eps"], h["momentum"], h["beta1"], h["beta2"], h["weight_decay"],
                               0.0, 1.0, [])

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        counted = self.KIND != "sgd"
        for group in self.param_groups:
            check_supported(self.KIND, group)
            keys = self._keys(group)
            flat = self._flat(group)
            if flat is not None:
                require_device(flat[0], "parameter")
                t = 0
                if counted:
                    st = self.state[group["params"][0]]["step"]  # one counter shared by the group
                    t = int(st)
                    st += 1
                self._update(group, flat[0], flat[1:-1], flat[-1], t)
                continue
            for p in group["params"]:
                if p.grad is None:
                    continue
                require_device(p, "parameter")
                state = self.state[p]
                if (keys and keys[0] not in state) or (counted and "step" not in state):
                    if counted:
                        state["step"] = torch.zeros((), dtype=torch.float32)
                    for k in keys:
                        state[k] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                t = 0
                if counted:
                    t = int(state["step"])
                    state["step"] += 1
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                if not p.is_contiguous():
                    raise RuntimeError(f"fall3 {type(self).__name__} needs contiguous parameters")
                self._update(group, p, [state[k] for k in keys], g, t)
        return loss


class RMSprop(_FlatOptimizer):
    """torch.optim.RMSprop(lr, alpha=0.99, eps=1e-8, weight_decay=0) — no momentum, not centred — as
    fall3::rmsprop_ (f3_rmsprop_step; weight_decay 0, the reference's call) or fall3::optim_ custom ops."""

    KIND = "rmsprop"

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False,
                 maximize=False):
        d = dict(lr=lr, alpha=alpha, eps=eps)
        # the keys beyond torch's three appear only when set, so a default group stays {lr, alpha, eps}
        for k, v in (("weight_decay", weight_decay), ("momentum", momentum), ("centered", centered),
                     ("maximize", maximize)):
            if v:
                d[k] = v
        check_supported("rmsprop", d)
        super().__init__(params, d)

    def _update(self, group, p, states, g, t):
        if group.get("weight_decay", 0) == 0:
            torch.ops.fall3.rmsprop_(p, states[0], g, group["lr"], group["alpha"], group["eps"], 1.0)
        else:
            super()._update(group, p, states, g, t)


class SGD(_FlatOptimizer):
    """torch.optim.SGD(lr, momentum, dampening=0, weight_decay, nesterov) as fall3::optim_."""

    KIND = "sgd"

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False):
        d = torch_defaults("sgd", lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                           nesterov=nesterov, maximize=maximize)
        check_supported("sgd", d)
        super().__init__(params, d)


class Adam(_FlatOptimizer):
    """torch.optim.Adam(lr, betas, eps, weight_decay) as fall3::optim_ (L2 decay added to the gradient)."""

    KIND = "adam"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *,
                 maximize=False):
        d = torch_defaults(self.KIND, lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                           maximize=maximize)
        check_supported(self.KIND, d)
        super().__init__(params, d)


class AdamW(Adam):
    """torch.optim.AdamW(lr, betas, eps, weight_decay=1e-2) as fall3::optim_ (decoupled decay)."""

    KIND = "adamw"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *,
                 maximize=False):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, maximize=maximize)


class CosineLRScheduler:
    """timm.scheduler.CosineLRScheduler as the reference builds it (model/optimizer.py:31; timm is
    not installed here, so its published schedule is restated): cycle_mul 1, decay_rate 1,
    cycle_limit 1, k_decay 1, warmup_prefix False, no noise.
      t <  warmup_t : lr = warmup_lr_init + t * (base_lr - warmup_lr_init) / warmup_t
      t <  t_initial: lr = lr_min + (base_lr - lr_min) * (1 + cos(pi * t / t_initial)) / 2
      otherwise     : lr = lr_min
    The warm-up value is applied at construction (so epoch 0 trains at warmup_lr_init) and
    step(epoch) sets the value for `epoch` (t_in_epochs; step_update(num_updates) otherwise)."""

    def __init__(self, optimizer, t_initial, lr_min=0.0, t_in_epochs=True, warmup_t=0, warmup_lr_init=0.0):
        self.optimizer = optimizer
        self.t_initial, self.lr_min, self.t_in_epochs = t_initial, lr_min, t_in_epochs
        self.warmup_t, self.warmup_lr_init = warmup_t, warmup_lr_init
        for g in optimizer.param_groups:
            g.setdefault("initial_lr", g["lr"])
        self.base_values = [g["initial_lr"] for g in optimizer.param_groups]
        self.warmup_steps = [(v - warmup_lr_init) / warmup_t for v in self.base_values] if warmup_t else []
        if warmup_t:
            self._set([warmup_lr_init] * len(self.base_values))

    def _get_lr(self, t):
        if t < self.warmup_t:
            return [self.warmup_lr_init + t * s for s in self.warmup_steps]
        if t < self.t_initial:
            return [self.lr_min + 0.5 * (v - self.lr_min) * (1 + math.cos(math.pi * t / self.t_initial))
                    for v in self.base_values]
        return [self.lr_min for _ in self.base_values]

    def _set(self, values):
        for g, v in zip(self.optimizer.param_groups, values):
            g["lr"] = v

    def step(self, epoch, metric=None):
        if self.t_in_epochs:
            self._set(self._get_lr(epoch))

    def step_update(self, num_updates, metric=None):
        if not self.t_in_epochs:
            self._set(self._get_lr(num_updates))

    def state_dict(self):
        return {k: v for k, v in self.__dict__.items() if k != "optimizer"}

    def load_state_dict(self, state):
        self.__dict__.update(state)


def build_optimizer(model, config):
    t = config.OPTIM.TYPE
    if t == "rmsprop":
        opt = RMSprop(model.parameters(), lr=config.OPTIM.LR)
    elif t == "sgd":
        opt = SGD(model.parameters(), lr=config.OPTIM.LR, momentum=config.OPTIM.MOMENTUM,
                  weight_decay=config.OPTIM.WEIGHT_DECAY)
    elif t == "adam":
        opt = Adam(model.parameters(), lr=config.OPTIM.LR, betas=config.OPTIM.BETAS, eps=config.OPTIM.EPS,
                   weight_decay=config.OPTIM.WEIGHT_DECAY)
    elif t == "adamw":
        opt = AdamW(model.parameters(), lr=config.OPTIM.LR, betas=config.OPTIM.BETAS, eps=config.OPTIM.EPS,
                    weight_decay=config.OPTIM.WEIGHT_DECAY)
    else:
        raise RuntimeError(f"Optimizer type [{t}] is not implemented.")
    if config.LR_SCHEDULER.TYPE is None:
        return opt, None
    if config.LR_SCHEDULER.TYPE == "cosine":
        c = config.LR_SCHEDULER
        return opt, CosineLRScheduler(opt, t_initial=c.T_INITIAL, lr_min=c.LR_MIN, t_in_epochs=c.T_IN_EPOCHS,
                                      warmup_t=c.WARMUP_T, warmup_lr_init=c.WARMUP_LR_INIT)
    raise RuntimeError(f"LR Scheduler type [{config.LR_SCHEDULER.TYPE}] is not implemented.")
