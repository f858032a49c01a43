"""AdamW over all parameters in ONE kernel launch (csrc/adamw.hip) -- the update `train_rqvae.py:136-138` of the reference asks for
(`AdamW(params=model.parameters(), lr, weight_decay)`: decoupled weight decay on every parameter, codebooks included).

A `torch.optim.Optimizer` with AdamW's constructor, `param_groups` and per-parameter state (`step`, `exp_avg`, `exp_avg_sq`), so that
`optimizer.state_dict()` / `load_state_dict()` -- the `"optimizer"` entry of the reference's checkpoints (train_rqvae.py:260-265) -- are
interchangeable with `torch.optim.AdamW`'s in both directions.  What differs is the launch: torch's fused kernel works on 64 K-element chunks
(18 workgroups for this model's 1.15 M parameters: 40-46 us per step, plus a launch that bumps the step counters); here 1 100 workgroups
update everything in a few microseconds behind a one-thread kernel that bumps the one device-side step counter -- which also makes the step replayable from a
captured hipGraph without torch's `capturable` machinery.  The hyper-parameters are kernel arguments: a captured graph replays the values
it was captured with (train_rqvae.py re-captures after every eager excursion; it has no scheduler).

The retrieval model's loop (reference train_decoder.py:147-151, 202-205) clips the global gradient norm and drives the learning rate with
`modules.scheduler.InverseSquareRootScheduler`; both change from step to step, so neither can be a kernel argument of a replayed step.
With `max_grad_norm` set or such a scheduler attached, step() runs the second entry point of csrc/adamw.hip instead
(`rqhip_adamw_tail_step`): the norm, the clip coefficient and the scheduled learning rate are formed on the device from device counters,
and are left in device tensors (`grad_norm`, `device_lr`) for logging without a host round trip."""
import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import RqHipError, check
from .ops import _RAW_DEVICE, _stream as ops_stream


# FlatAdamW's kernels write the parameters through raw pointers, which leaves their `_version` counters alone; whoever keeps
# something derived from parameter VALUES (modules/t5.py: the bf16 weight images) puts this count into its staleness key.
_generation = 0


def generation() -> int:
    """How many FlatAdamW.step() calls this process has made, over all optimizers."""
    return _generation


class FlatAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, amsgrad: bool = False, *,
                 maximize: bool = False, foreach: Optional[bool] = None, capturable: bool = False, differentiable: bool = False,
                 fused: Optional[bool] = None, max_grad_norm: Optional[float] = None) -> None:
        if amsgrad or maximize or differentiable:
            raise ValueError("FlatAdamW implements plain AdamW (no amsgrad / maximize / differentiable)")
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1):
            raise ValueError("invalid AdamW hyper-parameters")
        del foreach, capturable, fused          # accepted for signature compatibility: one kernel, always graph-safe
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=True, differentiable=False, fused=True)
        super().__init__(params, defaults)
        self._steps = {}        # group index -> the device float scalar every parameter of the group shares as state["step"]
        self._scratch = None
        self._cache = {}
        # the clip-and-schedule tail.  Kept out of param_groups: state_dict() stays torch.optim.AdamW's
        self.max_grad_norm = max_grad_norm      # None: no clipping; else the max_norm of clip_grad_norm_ (2-norm over ALL parameters)
        self._tail = {}         # group index -> [scalars (RQHIP_ADAMW_TAIL_SCALARS floats), lr_step (int64 scalar), workspace or None, views]
        self._schedule = {}     # group index -> (warm-up steps, base lr) of the attached inverse-square-root schedule

    def _tail_state(self, gi: int):
        ts = self._tail.get(gi)
        if ts is None:
            dev = self.param_groups[gi]["params"][0].device
            ts = [torch.zeros((_lib.ADAMW_TAIL_SCALARS,), dtype=torch.float32, device=dev), torch.zeros((), dtype=torch.int64, device=dev), None]
            ts += [ts[0][2], ts[0][4]]          # the views device_lr() and grad_norm hand out
            self._tail[gi] = ts
        return ts

    @property
    def grad_norm(self) -> torch.Tensor:
        """Device fp32 scalar: the 2-norm of all gradients of the last step() BEFORE clipping (what clip_grad_norm_ returns).  One
        tensor for the optimizer's lifetime, so a captured graph owns it; NaN after a step without clipping (not computed), 0 before the first."""
        return self._tail_state(0)[4]

    def device_lr(self, group_index: int = 0) -> torch.Tensor:
        """Device fp32 scalar: the learning rate the last step() of this group used (the tail entry point only)."""
        return self._tail_state(group_index)[3]

    def device_lr_step(self, group_index: int = 0) -> torch.Tensor:
        """Device int64 scalar: the schedule's counter, = scheduler.last_epoch + 1 under the one-scheduler-step-per-optimizer-step contract."""
        return self._tail_state(group_index)[1]

    def attach_schedule(self, group_index: int, warmup_steps: int, lr_step: int, base_lr: float) -> None:
        """modules.scheduler.InverseSquareRootScheduler calls this: from now on step() forms this group's learning rate on the device,
        lr = base_lr if lr_step <= warmup_steps else base_lr sqrt(warmup_steps) / sqrt(lr_step), and advances lr_step itself
        (`group["lr"]` is then the scheduler's host mirror, not an input).  The counter is FILLED with `lr_step`: no read-back, and
        legal next to a captured graph that owns the tensor.  load_state_dict() keeps the schedule attached."""
        if warmup_steps < 0:
            raise ValueError("warmup_steps must be >= 0")
        self._tail_state(group_index)[1].fill_(int(lr_step))
        self._schedule[group_index] = (int(warmup_steps), float(base_lr))

    def _shared_step(self, gi: int, group) -> torch.Tensor:
        """One step counter per group, on the device; parameters loaded from a torch AdamW checkpoint bring their own (all equal).
        CONTRACT (differs from torch.optim.AdamW, which counts per parameter): every parameter of a group takes part in every step() --
        a parameter whose .grad is None on some steps, or that receives its first gradient later than the others, is bias-corrected
        with the GROUP's count.  The RQ-VAE training loops of this package (every parameter gets a gradient every step) satisfy it."""
        st = self._steps.get(gi)
        live = [self.state[p]["step"] for p in group["params"] if p in self.state and "step" in self.state[p]]
        if st is None or any(s is not st for s in live):
            dev = group["params"][0].device
            start = max([float(s) for s in live if s is not st] + ([float(st)] if st is not None else [0.0])) if live else 0.0   # (host sync)
            st = torch.full((), start, dtype=torch.float32, device=dev)
            self._steps[gi] = st
            for p in group["params"]:
                if p in self.state:
                    self.state[p]["step"] = st
        return st

    @torch.no_grad()
    def step(self, closure=None):
        global _generation
        _generation += 1        # before anything can fail: a key that changes needlessly costs one refresh
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        clip = self.max_grad_norm is not None
        if clip and len(self.param_groups) > 1:
            raise ValueError("FlatAdamW: max_grad_norm clips by the norm over ALL parameters; it takes one param group")
        if clip and not float(self.max_grad_norm) > 0:
            raise ValueError("FlatAdamW: max_grad_norm must be positive (or None)")
        l = _lib.lib()
        for gi, group in enumerate(self.param_groups):
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            dev = ps[0].device
            if dev.type != "cuda":
                raise RqHipError("FlatAdamW updates ROCm device parameters (csrc/adamw.hip); use torch.optim.AdamW for host tensors")
            # the same parameters and the same (aligned) gradient buffers as last step -- every step of a training loop whose gradients
            # live in rqhip.dist.FlatGradReducer's flat buffer: the argument arrays, the validation and the state lookups of the first
            # such step stand (load_state_dict drops them); 11 parameters x 5 Python loops were a third of an eager step's optimizer time
            fast = (tuple([p.data_ptr() for p in ps]), tuple([p.grad.data_ptr() for p in ps]))
            arrs = self._cache.get(gi)
            step = self._steps.get(gi)
            if arrs is None or arrs[0] != fast or step is None:
                for p in ps:
                    if p.dtype != torch.float32 or not p.is_contiguous() or p.grad.dtype != torch.float32 or p.grad.is_sparse:
                        raise RqHipError("FlatAdamW: parameters and gradients must be contiguous float32 tensors")
                    st = self.state[p]
                    if "exp_avg" not in st:
                        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                        st["step"] = self._steps.get(gi, torch.zeros((), dtype=torch.float32, device=dev))
                        self._steps.setdefault(gi, st["step"])
                step = self._shared_step(gi, group)
                # (the kernel reads 16 bytes at a time: a gradient that is a misaligned view of someone's packed buffer is copied once
                # per step; rqhip.dist.FlatGradReducer pads its slices, so its views never take this branch)
                direct = all(p.grad.is_contiguous() and p.grad.data_ptr() % 16 == 0 for p in ps)
                grads = [p.grad if (p.grad.is_contiguous() and p.grad.data_ptr() % 16 == 0) else p.grad.clone(memory_format=torch.contiguous_format)
                         for p in ps]
                n = len(ps)
                vp = C.c_void_p * n
                numel = (C.c_int64 * n)(*[p.numel() for p in ps])
                arrs = (fast if direct else None, vp(*[p.data_ptr() for p in ps]), vp(*[g.data_ptr() for g in grads]),
                        vp(*[self.state[p]["exp_avg"].data_ptr() for p in ps]), vp(*[self.state[p]["exp_avg_sq"].data_ptr() for p in ps]),
                        numel, n, grads,      # (grads: keeps copies alive until the launch)
                        l.rqhip_adamw_tail_workspace_bytes(numel, n))      # (host arithmetic; used by the clipping tail only)
                self._cache[gi] = arrs
            b1, b2 = group["betas"]
            warmup, base_lr = self._schedule.get(gi, (-1, 0.0))      # (-1: no schedule, the lr is the argument)
            if clip or warmup >= 0:
                # the tail entry point: norm, clip coefficient and scheduled lr on the device (csrc/adamw.hip)
                scalars, lr_step = self._tail_state(gi)[:2]
                ws, ws_bytes = None, 0
                if clip:
                    if arrs[8] < 0:
                        check(_lib.EARG, "rqhip_adamw_tail_workspace_bytes")
                    ws = self._tail[gi][2]
                    if ws is None or ws.numel() * 4 < arrs[8] or ws.device != dev:
                        ws = self._tail[gi][2] = torch.empty((max(arrs[8] // 4, 1),), dtype=torch.float32, device=dev)
                    ws_bytes = ws.numel() * 4

                def launch():
                    check(l.rqhip_adamw_tail_step(arrs[1], arrs[2], arrs[3], arrs[4], arrs[5], arrs[6], step.data_ptr(), lr_step.data_ptr(),
                                                  scalars.data_ptr(), None if ws is None else ws.data_ptr(), ws_bytes,
                                                  float(self.max_grad_norm) if clip else 0.0, float(group["lr"]),
                                                  base_lr, warmup,
                                                  float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]), ops_stream()),
                          "rqhip_adamw_tail_step")
            else:
                if self._scratch is None or self._scratch.device != dev:
                    self._scratch = torch.zeros((2,), dtype=torch.float32, device=dev)

                def launch():
                    check(l.rqhip_adamw_step(arrs[1], arrs[2], arrs[3], arrs[4], arrs[5], arrs[6], step.data_ptr(), self._scratch.data_ptr(),
                                             float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                                             ops_stream()), "rqhip_adamw_step")
            if _RAW_DEVICE is not None and dev.index == _RAW_DEVICE():     # (the device context manager costs more than the launch)
                launch()
            else:
                with torch.cuda.device(dev):
                    launch()
        return loss

    def state_dict(self):
        """torch.optim.AdamW's format.  Every parameter gets its OWN copy of the step counter: the live one is shared by the group, and a
        torch AdamW that loaded aliased counters would advance the shared tensor once per parameter."""
        sd = super().state_dict()
        for st in sd["state"].values():
            if torch.is_tensor(st.get("step")):
                st["step"] = st["step"].detach().clone()
        return sd

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        self._steps, self._cache = {}, {}
        # the loaded per-parameter counters (all equal in an AdamW checkpoint) become the group's shared device scalar NOW -- reading
        # them back is a host sync, which the next step() may not do (it can run under hipGraph capture)
        for gi, group in enumerate(self.param_groups):
            if any(p in self.state and "step" in self.state[p] for p in group["params"]):
                self._shared_step(gi, group)
