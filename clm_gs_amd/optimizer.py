"""SelectiveAdam and UnifiedAdam with the attribute surface the model and engine touch
(optimizer.py:6-184 of the reference: .gpu_adam, .cpu_adam, .columns_lr, .param_groups,
.state, step/zero_grad)."""
import torch

from . import cpu_adam
from .clm_kernels import selective_adam_update
from .host import is_pinned


class SelectiveAdam(torch.optim.Adam):
    """Visibility-masked fused Adam (Taming-3DGS flavour: no bias correction)."""

    def __init__(self, params, eps, betas):
        super().__init__(params=params, eps=eps, betas=betas)

    @torch.no_grad()
    def step(self, visibility):
        N = visibility.numel()
        for group in self.param_groups:
            assert len(group["params"]) == 1, "more than one tensor in group"
            param = group["params"][0]
            if param.grad is None:
                continue
            state = self.state[param]
            if len(state) == 0:
                state["step"] = torch.tensor(0.0, dtype=torch.float32)
                state["exp_avg"] = torch.zeros_like(param, memory_format=torch.preserve_format)
                state["exp_avg_sq"] = torch.zeros_like(param, memory_format=torch.preserve_format)
            beta1, beta2 = group["betas"]
            selective_adam_update(param, param.grad, state["exp_avg"], state["exp_avg_sq"],
                                  visibility, group["lr"], beta1, beta2, group["eps"], N,
                                  param.numel() // N)


class UnifiedAdam(torch.optim.Optimizer):
    """Two independent Adams behind one interface: torch fused Adam (or SelectiveAdam) for the
    GPU-resident groups and FusedCPUAdam for the group named "parameters" (the [N,48] SH rows,
    pinned host or HBM-resident)."""

    def __init__(self, params, columns_sizes, columns_lr, lr=1e-3, bias_correction=True,
                 betas=(0.9, 0.999), eps=1e-15, weight_decay=0, amsgrad=False, adamw_mode=False,
                 fp32_optimizer_states=True, fused=False, sparse=False, state_tensors=None):
        params_device, params_rows = [], []
        for p in params:
            if p["name"] == "parameters":
                t = p["params"][0]
                assert t.is_cuda or is_pinned(t), "SH rows must be pinned host or device memory"
                params_rows.append(p)
            else:
                assert p["params"][0].is_cuda
                params_device.append(p)
        if sparse:
            self.gpu_adam = SelectiveAdam(params_device, eps=eps, betas=betas)
        else:
            self.gpu_adam = torch.optim.Adam(params_device, lr=0.0, eps=eps, fused=fused)
        self.cpu_adam = cpu_adam.FusedCPUAdam(
            params_rows, columns_sizes=columns_sizes, columns_lr=columns_lr, lr=0.0,
            bias_correction=bias_correction, betas=betas, eps=eps, weight_decay=weight_decay,
            amsgrad=amsgrad, adamw_mode=adamw_mode, fp32_optimizer_states=fp32_optimizer_states,
            state_tensors=state_tensors)
        self.columns_lr = self.cpu_adam.columns_lr
        self.param_groups = self.gpu_adam.param_groups + self.cpu_adam.param_groups
        self.state = self.gpu_adam.state | self.cpu_adam.state

    def _gpu_state(self, p):
        """torch.optim.Adam's own state of a GPU-resident parameter, created if empty."""
        st = self.gpu_adam.state[p]
        if len(st) == 0:
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def small_groups(self):
        """The four small-attribute groups in the kernels' order, their state created if empty."""
        groups = {g["name"]: g for g in self.gpu_adam.param_groups}
        order = [groups[n] for n in ("xyz", "opacity", "scaling", "rotation")]
        for g in order:
            self._gpu_state(g["params"][0])
        return order

    def small_pointers(self, order):
        """The p / exp_avg / exp_avg_sq pointer arrays of small_groups(), as the clmgs_adam_small_* entries take them."""
        import ctypes
        cols = ([], [], [])
        for g in order:
            p = g["params"][0]
            st = self.gpu_adam.state[p]
            assert p.is_contiguous() and st["exp_avg"].is_contiguous() and st["exp_avg_sq"].is_contiguous()
            for col, t in zip(cols, (p, st["exp_avg"], st["exp_avg_sq"])):
                col.append(t.data_ptr())
        return tuple((ctypes.c_void_p * 4)(*c) for c in cols)

    def _count_steps(self, groups):
        """Advances the step counter of every group of `groups` (one launch) and returns their new step indices."""
        cache = self.__dict__.setdefault("_gpu_steps", {})
        counters = [self._gpu_state(g["params"][0])["step"] for g in groups]
        for t in counters:
            if id(t) not in cache:  # one host read per (re)created state, then counted here
                cache.clear() if len(cache) > 64 else None
                cache[id(t)] = int(t.item())
            cache[id(t)] += 1
        if counters:
            torch._foreach_add_(counters, 1)  # torch-Adam's own counters stay what a torch .step() leaves
        self.state = self.gpu_adam.state | self.cpu_adam.state
        return [cache[id(t)] for t in counters]

    def advance_steps(self, groups):
        """The step counters of `groups` advance together: returns the step index they are at now."""
        steps = self._count_steps(groups)
        assert all(s == steps[0] for s in steps), "the groups step together"
        return steps[0]

    @torch.no_grad()
    def gpu_step_scaled(self, grad_scale=1.0):
        """Dense Adam of the GPU-resident groups through clmgs_adam_rows: gradient scale (the
        engine's `grad /= bsz`), update and gradient zeroing in ONE pass per tensor instead of
        torch's three (div, fused Adam, fresh zeros next batch).  State stays in
        torch.optim.Adam's own layout (step / exp_avg / exp_avg_sq per parameter), so the
        densification surgery, capture / restore and a later torch .step() keep working; same
        bias-corrected formula as torch (step_size = lr / bc1, denom = sqrt(v) / sqrt(bc2) + eps)."""
        from .clm_kernels import adam_rows
        assert not isinstance(self.gpu_adam, SelectiveAdam)
        stepped = [g for g in self.gpu_adam.param_groups if g["params"][0].grad is not None]
        for group, step in zip(stepped, self._count_steps(stepped)):  # (each group at its own step index)
            p = group["params"][0]
            st = self.gpu_adam.state[p]
            # one learning rate per tensor -> the [N,d] layout is irrelevant: stream it as float4 rows
            cols = 4 if p.numel() % 4 == 0 else 1
            key = (cols, float(group["lr"]))
            lrs = self.__dict__.setdefault("_col_lr_cache", {})
            if key not in lrs:
                if len(lrs) > 256:
                    lrs.clear()
                lrs[key] = torch.full((cols,), float(group["lr"]), dtype=torch.float32, device=p.device)
            b1, b2 = group["betas"]
            adam_rows(p.data.view(-1, cols), p.grad.view(-1, cols), st["exp_avg"].view(-1, cols),
                      st["exp_avg_sq"].view(-1, cols), None, lrs[key], b1, b2, group["eps"], step, True,
                      float(grad_scale), True)

    @torch.no_grad()
    def gpu_step_packed(self, packed_p, packed_g, grad_scale=1.0, g_stamp=None, cur_step=0, row_range=None):
        """Dense Adam of the four GPU-resident tensors from the packed [N,12] gradient table
        (clmgs_adam_small_packed): updates p / exp_avg / exp_avg_sq of every group in place,
        refreshes the packed parameter mirror and zeroes the gradient table, all in one pass.
        g_stamp / cur_step: first-touch gradient table (only rows stamped cur_step carry a gradient;
        nothing is zeroed).  row_range = (lo, hi): only these rows are stepped (camera-DP: the small attributes are
        computed by the owner of a row range, clm_offload/gaussian_model.py small_owner); the step counters advance
        as usual -- they are per tensor, and every rank steps its range at every batch."""
        import ctypes
        from . import _lib
        assert not isinstance(self.gpu_adam, SelectiveAdam)
        order = self.small_groups()
        step = self.advance_steps(order)
        ps, ms, vs = self.small_pointers(order)
        g0 = order[0]
        lo, hi = (0, -1) if row_range is None else (int(row_range[0]), int(row_range[1]))
        _lib.check(_lib.lib().clmgs_adam_small_packed_range(
            _lib.stream(), int(packed_p.shape[0]), lo, hi, ps, ms, vs,
            (ctypes.c_double * 4)(*[float(g["lr"]) for g in order]),
            _lib.dptr(packed_p), _lib.dptr(packed_g), float(g0["betas"][0]), float(g0["betas"][1]),
            float(g0["eps"]), int(step), 1, float(grad_scale),
            None if g_stamp is None else _lib.dptr(g_stamp, torch.int32), int(cur_step)))

    def get_all_states(self):
        return [self.gpu_adam.state, self.cpu_adam.state]

    def zero_grad(self, set_to_none=False):
        self.gpu_adam.zero_grad(set_to_none)
        self.cpu_adam.zero_grad(set_to_none)

    def step(self, closure=None):
        self.gpu_adam.step()
        self.cpu_adam.step()
        self.state = self.gpu_adam.state | self.cpu_adam.state
