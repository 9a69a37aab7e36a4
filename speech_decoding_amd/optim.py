"""Adam over all parameter tensors in ONE kernel launch (same update rule and defaults as the
`torch.optim.Adam(params, lr=...)` of train.py:161-163; complex parameters are stepped through their real
view, exactly as PyTorch does).  Optional: the stock optimiser works unchanged with these modules."""
from __future__ import annotations

import ctypes as C

import torch

from . import lib as L


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        L.load()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            items = []
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda:
                    raise L.SdaError("FusedAdam needs device parameters (no CPU path)")
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                real = (lambda t: torch.view_as_real(t) if t.is_complex() else t)
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                items.append((real(p.data), real(g), real(st["exp_avg"]), real(st["exp_avg_sq"]), st["step"]))
            if not items:
                continue
            steps = {it[4] for it in items}
            for stp in sorted(steps):                       # parameters that joined later have their own step count
                sub = [it for it in items if it[4] == stp]
                raw, max_n = adam_table([it[:4] for it in sub])
                from .ops import UPLOADER
                # gradient tensors recur at the same addresses in steady state: the table is then a cache hit
                table = UPLOADER.upload(("adam", id(self)), raw, sub[0][0].device)
                b1, b2 = group["betas"]
                L.check(L.load().sda_adam_multi(table.data_ptr(), len(sub), max_n, float(group["lr"]),
                                                float(b1), float(b2), float(group["eps"]), int(stp),
                                                torch.cuda.current_stream().cuda_stream), "adam_multi")
                self._keep = (table, [s[1] for s in sub])     # keep the table / contiguous grads alive until the next step
        return loss


def adam_table(items):
    """The sda_adam_desc array of [(param, grad, exp_avg, exp_avg_sq) real fp32 views] as uint8 for the uploader, and max n."""
    import numpy as np
    arr = (L.AdamDesc * len(items))()
    for i, (pp, gg, m, v) in enumerate(items):
        arr[i].param, arr[i].grad, arr[i].exp_avg, arr[i].exp_avg_sq = pp.data_ptr(), gg.data_ptr(), m.data_ptr(), v.data_ptr()
        arr[i].n = pp.numel()
        arr[i].aligned = int(all(t.data_ptr() % 16 == 0 for t in (pp, gg, m, v)))
    return np.frombuffer(bytes(arr), dtype=np.uint8), max(int(a.n) for a in arr)


def _real(t):
    return torch.view_as_real(t) if t.is_complex() else t


class GuardedAdam(torch.optim.Optimizer):
    """FusedAdam behind a gradient guard that lives on the device: global-norm clipping (torch.nn.utils.clip_grad_norm_'s rule)
    and the loss scaler's overflow guard (amp.LossScaler's rules) without a host read-back.

        opt = GuardedAdam(params, lr=3e-4, max_grad_norm=1.0, loss_scale=1024.0, dynamic=True)
        opt.zero_grad(); opt.scale(loss).backward(); opt.step()          # nothing here waits for the device

    step() is exactly three launches on the current stream: the sum of squares and non-finite count of every gradient
    (sda_grad_sumsq_multi), the decision (sda_grad_guard_finish: skip / scale update / clip coefficient / bias corrections, into
    a 16-double device state), and Adam on grad * coefficient (sda_adam_multi_guarded; it writes nothing on a skipped step).

    Contract:
      * ONE step count for all tensors, kept on the device: the tensors that have a gradient at the first step() are the members;
        a parameter that gets its first gradient later raises.  One parameter group.
      * `.grad` is left as backward wrote it: still multiplied by the loss scale, not clipped.  Read `last_coef` for the factor.
      * A non-finite gradient skips the step whatever the dtype (loss_scale 1, dynamic False for bf16 / fp32): parameters, moments
        and the step count keep their bits.  clip_grad_norm_ + Adam would write NaN into every parameter instead.
      * loss_scale, skipped_steps, steps_taken, last_grad_norm, last_coef read the device state back (a synchronisation each):
        they are for logging, once per epoch.
      * max_scale defaults to max(loss_scale, 2^24), amp.LossScaler's rule; max_grad_norm None (or <= 0, or inf): no clipping.
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, loss_scale=1.0, dynamic=False,
                 growth_interval=2000, max_scale=None):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        if len(self.param_groups) != 1:
            raise L.SdaError("GuardedAdam: one parameter group (one device step count, one launch)")
        if not float(loss_scale) >= 1.0 or int(growth_interval) < 0:
            raise L.SdaError("GuardedAdam: loss_scale >= 1 and growth_interval >= 0")
        L.load()
        self.max_grad_norm = 0.0 if max_grad_norm is None else float(max_grad_norm)
        self.dynamic = bool(dynamic)
        self.growth_interval = int(growth_interval)
        self.max_scale = max(float(loss_scale), 2.0 ** 24) if max_scale is None else float(max_scale)
        self._init_scale = float(loss_scale)
        self._guard = None            # the device state (lib.GUARD_STATE doubles), made on the parameters' device at first use
        self._members = None          # ids of the parameters of the first step
        self._table_key = None        # the addresses the cached descriptor table was built from
        self._table = self._partials = None

    def _state_vector(self, device=None):
        if self._guard is None:
            if device is None:
                device = next(p.device for p in self.param_groups[0]["params"])
            if device.type != "cuda":
                raise L.SdaError("GuardedAdam needs device parameters (no CPU path)")
            host = torch.zeros(L.GUARD_STATE, dtype=torch.float64)
            host[L.GUARD_SCALE] = self._init_scale
            self._guard = host.to(device)
        return self._guard

    def scale(self, loss: torch.Tensor) -> torch.Tensor:
        """loss x the current loss scale, read on the device (fp32 like the loss: the product LossScaler.scale makes)."""
        return loss * self._state_vector(loss.device)[L.GUARD_SCALE].to(loss.dtype)

    def set_loss_scale(self, value: float) -> None:
        """Overwrite the device's loss scale (a device fill, no synchronisation): what `scaler.scale_value = x` is to LossScaler."""
        if not float(value) >= 1.0:
            raise L.SdaError("GuardedAdam: loss_scale >= 1")
        self._state_vector()[L.GUARD_SCALE] = float(value)

    @torch.no_grad()
    def step(self, closure=None):
        from . import ops
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group = self.param_groups[0]
        with_grad = [p for p in group["params"] if p.grad is not None]
        if not with_grad:
            return loss
        ids = [id(p) for p in with_grad]
        if self._members is None:
            self._members = set(ids)
        elif not self._members.issuperset(ids):
            raise L.SdaError("GuardedAdam: a parameter got its first gradient after the first step (there is one device step count)")
        items = []
        for p in with_grad:
            if not p.is_cuda:
                raise L.SdaError("GuardedAdam needs device parameters (no CPU path)")
            st = self.state[p]
            if not st:
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
            items.append((_real(p.data), _real(g), _real(st["exp_avg"]), _real(st["exp_avg_sq"])))
        device = items[0][0].device
        state = self._state_vector(device)
        key = tuple(t.data_ptr() for it in items for t in it)
        if key != self._table_key:        # gradient tensors recur at the same addresses in steady state: nothing is rebuilt then
            raw, max_n = adam_table(items)
            n = len(items)
            parts = ops.grad_guard_parts(n, max_n)
            if self._partials is None or self._partials.numel() != parts or self._partials.device != device:
                self._partials = torch.empty(parts, dtype=torch.float64, device=device)
            self._table = (ops.UPLOADER.upload(("guarded_adam", id(self)), raw, device), n, max_n, parts // (2 * n))
            self._table_key = key
        table, n, max_n, gx = self._table
        b1, b2 = group["betas"]
        ops.grad_sumsq_multi(table, n, max_n, self._partials)
        ops.grad_guard_finish(self._partials, n, gx, state, self.max_grad_norm, b1, b2, self.growth_interval, self.max_scale, self.dynamic)
        ops.adam_multi_guarded(table, n, max_n, group["lr"], b1, b2, group["eps"], state)
        self._keep = [it[1] for it in items]          # contiguous copies of gradients stay alive until the next step
        return loss

    def _read(self, slot):
        return float(self._state_vector()[slot])

    loss_scale = property(lambda self: self._read(L.GUARD_SCALE))
    skipped_steps = property(lambda self: int(self._read(L.GUARD_SKIPPED)))
    steps_taken = property(lambda self: int(self._read(L.GUARD_STEP)))
    last_grad_norm = property(lambda self: self._read(L.GUARD_NORM))
    last_coef = property(lambda self: self._read(L.GUARD_COEF))

    def state_dict(self):
        """torch's optimizer state (the moments by parameter index, the group's settings) plus "guard": a copy of the device state."""
        out = super().state_dict()
        out["guard"] = self._state_vector().clone()
        return out

    def load_state_dict(self, state_dict):
        state_dict = dict(state_dict)
        guard = state_dict.pop("guard")
        super().load_state_dict(state_dict)
        for st in self.state.values():                # (torch hands a tensor that needs no cast over as it is: two optimisers
            for k, v in st.items():                   # loaded from one dict would step the same moments)
                if torch.is_tensor(v):
                    st[k] = v.clone()
        self._state_vector().copy_(guard)
        self._members = {id(p) for p in self.param_groups[0]["params"] if p in self.state} or None
        self._table_key = None                        # the moments are new tensors
