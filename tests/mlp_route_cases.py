"""The MLP stacks, row counts, variants and switches that tests/test_host_logic.py (which kernel routes they reach: no GPU) and
tests/test_gpu_mlp_routes.py (what they compute, against fp64) share -- a plain helper module, imported by both.

rqhip/linear.py:plan_layer decides the kernel of every layer's forward, data gradient and weight gradient; modules/encoder.py:_MLPStack
hands state from layer to layer according to the NEIGHBOUR's route (maxima, masks, job lists).  The shipped stacks put every layer of a
stack on the same family of routes; the stacks below mix them.  Widths are input -> ... -> output, a ReLU behind every layer but the last.
S1-S4 and M1-M5 are the stacks the table was drawn up with; M6-M8 were added for neighbour pairs the shape rules allow and none of
those reaches: a split data gradient feeding a library weight gradient (M6), a seam forward feeding a library forward (M7) and a seam
forward feeding the other seam forward (M8).
"""
import functools
from contextlib import contextmanager
from typing import List, NamedTuple, Optional, Tuple

import torch

STACKS = {
    "S1": (768, 512, 256, 128, 32),      # shipped encoder (anchor)
    "S2": (32, 128, 256, 512, 768),      # shipped decoder
    "S3": (768, 512, 256, 128, 64),      # configuration 3's latent: at 4096 rows and more the 128 <-> 64 layers mix library, split, fp32-MFMA
    "S4": (64, 128, 256, 512, 768),
    "M1": (256, 384, 208, 128, 32),      # a library layer between split layers; split GEMMs of reduction depth 208; the narrow 128-column tile
    "M2": (768, 96, 64, 32),             # 96 and 64 wide: small kernels plus a 64 x 96 job; above, a split data gradient under a library forward
    "M3": (256, 128, 100, 64, 32),       # 100 breaks the stack's job table: one-job launches between library neighbours
    "M4": (256, 128, 32, 64),            # a ReLU behind 128 -> 32: the documented difference between stack node and per-layer path
    "M5": (128,) * 10,                   # nine layers: more than one job table holds; 128 x 128 weight gradients on the fp32-MFMA kernel
    "M6": (100, 128, 256, 64),           # a split data gradient, masked in its epilogue, feeding a LIBRARY weight gradient (128 x 100)
    "M7": (32, 128, 64),                 # forward SEAM_OUT -> LIBRARY: the seam kernel's output read by a library GEMM
    "M8": (32, 128, 32),                 # forward SEAM_OUT -> SEAM_IN
}
ROWS = (1, 33, 640, 4095, 4096, 4097)    # both sides of the 4096-row threshold, ragged tiles, a single row
SWITCH_ROWS = (640, 4097)

# name -> (function of rqhip.linear, value, the stack it runs on)
SWITCHES = {
    "arith_bf16x3": ("use_arith", "bf16x3", "S3"),
    "arith_fp32": ("use_arith", "fp32", "S1"),
    "no_small": ("use_small_kernels", False, "M2"),
    "no_wgrad_jobs": ("use_wgrad_jobs", False, "S2"),
    "no_chain": ("use_chain_gemms", False, "S2"),
    "no_split": ("use_split_gemms", False, "M1"),
    "no_narrow": ("use_narrow_tiles", False, "S4"),
    "no_wgrad_batch": ("use_wgrad_batch", False, "S1"),
}


class Case(NamedTuple):
    stack: str
    rows: int
    input_grad: bool               # the input requires a gradient
    frozen: Tuple[int, ...] = ()   # layers whose weight does not
    switch: Optional[str] = None   # key of SWITCHES

    @property
    def id(self) -> str:
        tag = f"{self.stack}-{self.rows}-{'dx' if self.input_grad else 'nodx'}"
        if self.frozen:
            tag += "-frozen" + "".join(str(i) for i in self.frozen)
        return tag + (f"-{self.switch}" if self.switch else "")

    @property
    def widths(self) -> Tuple[int, ...]:
        return STACKS[self.stack]

    @property
    def n_layers(self) -> int:
        return len(self.widths) - 1


def cases() -> List[Case]:
    """Every case, those of one (stack, rows) next to each other (they share one fp64 reference)."""
    out = []
    for stack, widths in STACKS.items():
        n = len(widths) - 1
        for rows in ROWS:
            out += [Case(stack, rows, True), Case(stack, rows, False)]
            if stack in ("S1", "M1"):
                out += [Case(stack, rows, True, (0, 2)), Case(stack, rows, False, (0, 2)), Case(stack, rows, True, tuple(range(n)))]
            if rows in SWITCH_ROWS:
                out += [Case(stack, rows, True, (), name) for name, (_, _, on) in SWITCHES.items() if on == stack]
    return out


@contextmanager
def switched(name: Optional[str]):
    """The module switch of SWITCHES[name] flipped, and restored whatever happens."""
    from rqhip import linear
    if name is None:
        yield
        return
    fn, value, _ = SWITCHES[name]
    before = getattr(linear, fn)(value)
    try:
        yield
    finally:
        getattr(linear, fn)(before)


def _needs(case: Case):
    n = case.n_layers
    need_w = [i not in case.frozen for i in range(n)]
    need_in = [case.input_grad or any(need_w[:i]) for i in range(n)]
    return need_w, need_in


def stack_plans(case: Case, aligned: bool = True):
    """(plans, stack_jobs) as modules/encoder.py:_MLPStack.forward computes them (under the switches in force)."""
    from rqhip import linear
    w, n = case.widths, case.n_layers
    need_w, need_in = _needs(case)
    stack_jobs = linear.wgrad_jobs_ok(case.rows, [(w[i + 1], w[i]) for i in range(n) if need_w[i]])
    return [linear.plan_layer(case.rows, w[i + 1], w[i], relu=i + 1 < n, operands_aligned=aligned, need_dgrad=need_in[i],
                              need_wgrad=need_w[i], stack_jobs=stack_jobs) for i in range(n)], stack_jobs


def layerwise_plans(case: Case):
    """What the per-layer path runs: rqhip/linear.py:forward, input_grad and weight_grad each ask plan_layer on their own -- input_grad
    is not told about the ReLU, weight_grad knows no stack."""
    from rqhip import linear
    w, n, R = case.widths, case.n_layers, linear.Route
    need_w, need_in = _needs(case)
    plans = []
    for i in range(n):
        relu = i + 1 < n
        fwd = linear.plan_layer(case.rows, w[i + 1], w[i], relu=relu, operands_aligned=True, need_dgrad=False, need_wgrad=False).fwd
        dgrad = linear.plan_layer(case.rows, w[i + 1], w[i], relu=False, operands_aligned=True, need_wgrad=False).dgrad if need_in[i] else R.NONE
        wgrad = linear.plan_layer(case.rows, w[i + 1], w[i], relu=relu, operands_aligned=True, need_dgrad=False).wgrad if need_w[i] else R.NONE
        plans.append(linear.LayerPlan(fwd, dgrad, wgrad))
    return plans


def same_kernels(case: Case) -> bool:
    """Do stack node and per-layer path run the same kernels for this case (then their results are equal bit for bit)?  Both sides
    name a layer's fp16 weight gradient by plan_layer's route, batched or not, so a batched launch does not show here: it cuts its
    layers into other row ranges than a layer's own launch, and the caller compares bits with use_wgrad_batch(False)."""
    return [tuple(p) for p in stack_plans(case)[0]] == [tuple(p) for p in layerwise_plans(case)]


# ---- inputs and the fp64 reference ------------------------------------------------------------------------------------------------------
KINK_MARGIN = 2.0 ** -17     # a pre-activation this close to zero (relative to its layer's largest): the ReLU mask is anybody's guess
MAX_ZEROED = 0.10            # of a case's rows may lose their upstream gradient for that
_SEED = {}                   # (stack, rows) -> seed, where the default one zeroes too many rows


class Reference(NamedTuple):
    weights: List[torch.Tensor]     # fp32 [n_out, n_in], default nn.Linear initialisation
    x: torch.Tensor                 # fp32 [rows, widths[0]], unit-norm rows
    gout: torch.Tensor              # fp32 [rows, widths[-1]], randn / rows, zero in the ambiguous rows
    zeroed: float                   # fraction of ambiguous rows
    out: torch.Tensor               # fp64: the stack's output, every weight gradient, the input gradient
    gws: List[torch.Tensor]
    gx: torch.Tensor


@functools.lru_cache(maxsize=3)
def reference(stack: str, rows: int) -> Reference:
    """The stack as a chain of fp64 matmuls and ReLUs on the CPU, through fp64 autograd, from fp32 weights and inputs."""
    widths = STACKS[stack]
    gen = torch.Generator().manual_seed(_SEED.get((stack, rows), 7919 * list(STACKS).index(stack) + rows))
    weights = []
    for k, n in zip(widths[:-1], widths[1:]):     # nn.Linear's default: kaiming_uniform_(a = sqrt(5)) = U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))
        weights.append((torch.rand(n, k, generator=gen) * 2 - 1) * k ** -0.5)
    x = torch.nn.functional.normalize(torch.randn(rows, widths[0], generator=gen), dim=-1)
    gout = torch.randn(rows, widths[-1], generator=gen) / rows
    w64 = [w.double().requires_grad_(True) for w in weights]
    x64 = x.double().requires_grad_(True)
    h, ambiguous = x64, torch.zeros(rows, dtype=torch.bool)
    for i, w in enumerate(w64):
        z = h @ w.t()
        if i + 1 < len(w64):
            ambiguous |= (z.detach().abs() <= KINK_MARGIN * z.detach().abs().max()).any(dim=1)
            h = torch.relu(z)
        else:
            h = z
    gout = gout.clone()
    gout[ambiguous] = 0.0
    grads = torch.autograd.grad(h, [x64, *w64], gout.double())
    return Reference(weights, x, gout, float(ambiguous.float().mean()), h.detach(), list(grads[1:]), grads[0])


def rel_err(got: torch.Tensor, ref64: torch.Tensor) -> float:
    """max |got - ref| / max |ref|, in fp64 on the CPU."""
    scale = ref64.abs().max().item()
    return (got.detach().double().cpu() - ref64).abs().max().item() / scale if scale > 0 else float(got.detach().abs().max().item() > 0)
