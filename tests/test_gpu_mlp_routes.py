"""The MLP stack on every kernel route against an fp64 reference (cases: tests/mlp_route_cases.py; which routes they reach is checked
without a GPU in tests/test_host_logic.py).

For every case the stack runs as ONE autograd node (`MLP._run`, modules/encoder.py:_MLPStack) and layer by layer (`MLP._run_layerwise`),
forward and backward.  Reference: the same chain of matmuls and ReLUs in fp64 on the CPU through fp64 autograd, from the same fp32
weights (default nn.Linear initialisation), unit-norm input rows and upstream gradient randn / rows.

ReLU kinks: a pre-activation within rounding of zero lets two correct evaluations disagree about the mask, i.e. about one whole row term
of a weight gradient.  Rows with |z| <= 2^-17 max|z of that layer| somewhere in the fp64 reference get a ZERO upstream gradient in every
run (their masks then cannot matter; their forward output is still compared); at most 10 % of a case's rows, asserted.

Gate, for the output, every weight gradient and the input gradient: e = max|got - ref64| / max|ref64| <= F * e_lib, where e_lib is the
same figure for the same stack as plain fp32 torch operators on the GPU (F.linear, relu, autograd).  F, per kind of tensor, is twice the
worst e / e_lib measured over all cases on an MI355X, rounded up to a power of two: profiles/mlp_routes_error.txt (worst ratios: output
1.50, weight gradients 2.10, input gradient 1.36; none above 4).  A mask or maxima mistake is an error of order 1, a million times e_lib,
and fails any such F.

Stack node against per-layer path: where both run the same kernels (mlp_route_cases.same_kernels, from the plans) every tensor is equal
BIT FOR BIT -- rqhip/linear.py's claim -- with the node's batched weight-gradient launch off, as in tests/test_gpu_modules.py.  Where
they differ by design only the fp64 gate applies: stack M4 (a ReLU behind 128 -> 32: the per-layer data gradient does not know of it) and
stack M2 below 4096 rows (64-wide layers: jobs of the stack's table, library on the per-layer path)."""
import functools

import pytest
import torch

import mlp_route_cases as mc

pytestmark = pytest.mark.gpu

F = {"out": 4.0, "dW": 8.0, "dx": 4.0}      # profiles/mlp_routes_error.txt


@functools.lru_cache(maxsize=3)
def _device_side(stack, rows):
    """(x, gout) on the GPU and e_lib = {tensor name: error of the plain fp32 torch run against fp64} of one (stack, rows)."""
    ref = mc.reference(stack, rows)
    x, gout = ref.x.cuda(), ref.gout.cuda()
    ws = [w.cuda().requires_grad_(True) for w in ref.weights]
    xg = x.clone().requires_grad_(True)
    h = xg
    for i, w in enumerate(ws):
        h = torch.nn.functional.linear(h, w)
        if i + 1 < len(ws):
            h = torch.relu(h)
    grads = torch.autograd.grad(h, [xg, *ws], gout)
    e_lib = {"out": mc.rel_err(h, ref.out), "dx": mc.rel_err(grads[0], ref.gx)}
    e_lib.update({f"dW{i}": mc.rel_err(g, r) for i, (g, r) in enumerate(zip(grads[1:], ref.gws))})
    return x, gout, e_lib


def _model(case, ref):
    from modules.encoder import MLP
    w = case.widths
    mlp = MLP(w[0], list(w[1:-1]), w[-1]).cuda()
    lins = [m for m in mlp.mlp if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        for lin, weight in zip(lins, ref.weights):
            lin.weight.copy_(weight)
    for i, lin in enumerate(lins):
        lin.weight.requires_grad_(i not in case.frozen)
    return mlp, lins


def _run(fn, mlp, lins, x, gout, input_grad, grad_seen=None):
    """(output, [weight gradient or None], input gradient or None) of one forward + backward through `fn` (MLP._run / MLP._run_layerwise)."""
    for lin in lins:
        lin.weight.grad = None
    xx = x.detach().requires_grad_(input_grad)      # (same storage, same address)
    y = fn(xx, list(mlp.mlp))
    if grad_seen is not None:
        y.register_hook(lambda g: grad_seen.append(g.data_ptr() % 16))
    y.backward(gout)
    return y.detach(), [lin.weight.grad for lin in lins], xx.grad


def _gate(tag, case, got, ref, e_lib):
    out, gws, gx = got
    figures = [("out", mc.rel_err(out, ref.out), e_lib["out"])]
    for i, (gw, r) in enumerate(zip(gws, ref.gws)):
        if i in case.frozen:
            assert gw is None, f"{case.id} {tag}: frozen weight {i} got a gradient"
        else:
            figures.append((f"dW{i}", mc.rel_err(gw, r), e_lib[f"dW{i}"]))
    if case.input_grad:
        figures.append(("dx", mc.rel_err(gx, ref.gx), e_lib["dx"]))
    else:
        assert gx is None
    for name, e, el in figures:
        print(f"MLPROUTE {case.id} {tag} {name} e={e:.4e} e_lib={el:.4e} ratio={e / el if el > 0 else (0.0 if e == 0 else float('inf')):.3f}")
    bad = [f for f in figures if not f[1] <= F[f[0].rstrip('0123456789')] * f[2]]
    assert not bad, f"{case.id} {tag}: (tensor, e, e_lib) beyond F x e_lib, F = {F}: {bad}"


def _assert_equal_bits(case, a, b):
    assert torch.equal(a[0], b[0]), f"{case.id}: outputs of stack node and per-layer path differ"
    for i, (u, v) in enumerate(zip(a[1], b[1])):
        assert (u is None and v is None) or torch.equal(u, v), f"{case.id}: dW{i} of stack node and per-layer path differ"
    assert (a[2] is None and b[2] is None) or torch.equal(a[2], b[2]), f"{case.id}: input gradients of stack node and per-layer path differ"


@pytest.mark.parametrize("case", mc.cases(), ids=lambda c: c.id)
def test_mlp_stack_on_every_route_matches_fp64(case):
    from rqhip import linear
    ref = mc.reference(case.stack, case.rows)
    assert ref.zeroed <= mc.MAX_ZEROED, f"{case.id}: {ref.zeroed:.1%} of the rows sit on a ReLU kink"
    x, gout, e_lib = _device_side(case.stack, case.rows)
    mlp, lins = _model(case, ref)
    with mc.switched(case.switch):
        node = _run(mlp._run, mlp, lins, x, gout, case.input_grad)
        layerwise = _run(mlp._run_layerwise, mlp, lins, x, gout, case.input_grad)
        same = mc.same_kernels(case)
        node_unbatched = node
        if same and any(p.wgrad == linear.Route.F16_SPLIT_BATCHED for p in mc.stack_plans(case)[0]):
            before = linear.use_wgrad_batch(False)     # (a batched launch cuts its layers into other row ranges: same arithmetic, another tree)
            try:
                node_unbatched = _run(mlp._run, mlp, lins, x, gout, case.input_grad)
            finally:
                linear.use_wgrad_batch(before)
    _gate("node", case, node, ref, e_lib)
    _gate("layerwise", case, layerwise, ref, e_lib)
    if same:
        _assert_equal_bits(case, node_unbatched, layerwise)


_OPS_WITH_ACTIVATIONS = ("maxima", "gemm_split_ex", "linear_small", "rq_seam", "linear_wgrad", "linear_wgrad_f16_batch", "linear_wgrad_jobs")


def _off_by_four_bytes(t):
    """A contiguous copy of `t` that starts 4 bytes behind a 16-byte boundary."""
    v = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)[1:].view_as(t)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("rows", [640, 4097])
@pytest.mark.parametrize("which", ["input", "upstream_gradient"])
def test_misaligned_operands_compute_and_no_kernel_sees_them(which, rows, monkeypatch):
    """A contiguous fp32 operand whose address is not a multiple of 16 (a view into a larger buffer): the stack node re-homes it, the
    per-layer path sends its layer to the library; both compute (the node used to raise at 4096 rows and more, from rqhip_maxima), and
    no entry point of rqhip.ops is handed a misaligned matrix."""
    from rqhip import ops
    case = mc.Case("S1", rows, True)
    ref = mc.reference(case.stack, case.rows)
    x, gout, e_lib = _device_side(case.stack, case.rows)
    x, gout = (_off_by_four_bytes(x), gout) if which == "input" else (x, _off_by_four_bytes(gout))
    mlp, lins = _model(case, ref)
    seen = []

    def spy(name, fn):
        def matrices(v):
            if isinstance(v, torch.Tensor):
                return [v] if (v.dtype == torch.float32 and v.dim() == 2) else []
            if isinstance(v, (list, tuple)):
                return [t for u in v for t in matrices(u)]
            return []

        def call(*args, **kwargs):
            seen.extend((name, t.data_ptr() % 16) for t in matrices(list(args) + list(kwargs.values())))
            return fn(*args, **kwargs)
        return call

    for name in _OPS_WITH_ACTIVATIONS:
        monkeypatch.setattr(ops, name, spy(name, getattr(ops, name)))
    for tag, fn in (("node", mlp._run), ("layerwise", mlp._run_layerwise)):
        grads_in = []
        got = _run(fn, mlp, lins, x, gout, True, grads_in)
        assert grads_in == [4 if which == "upstream_gradient" else 0]       # the gradient reached the stack as it was given
        _gate(f"{tag}-misaligned-{which}", case, got, ref, e_lib)
    assert seen and all(rem == 0 for _, rem in seen), sorted({s for s in seen if s[1]})
