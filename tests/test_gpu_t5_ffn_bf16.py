"""The "bf16" arithmetic of the fused T5 feed-forward on the GPU: ops.t5_ffn_fwd / ops.t5_ffn_bwd with arith="bf16"
(csrc/t5_ffn.hip, rqhip_t5_ffn_*_bf16) against fp64 on operands rounded to bf16 on the host (`.to(torch.bfloat16)`:
nearest even, as v_cvt_pk_bf16_f32).

The kernel's own intermediates are used at every stage, so no stage inherits another's rounding flips:
  h     against relu(bf(x) @ bf(wi).T)
  y     against bf(hd) @ bf(wo).T, hd = keep ? h * s : 0 restated in fp32 from the kernel's h and
        ops.t5_attention_dropout_keep
  g     (the workspace, return_g) against on ? (bf(d_y) @ bf(wo)) * s : 0, on = (kernel's h > 0) and keep
  d_x   against bf(g) @ bf(wi)          d_wi against bf(g).T @ bf(x)          d_wo against bf(d_y).T @ bf(hd)

Gate, elementwise: |kernel - ref64| <= (K + 8) * 2^-23 * (|a| @ |b|) with K the reduction length and |a| @ |b| in fp64
on the rounded operands.  Products of two bf16 values are exact in fp32; any order of K fp32 additions errs by at most
(K - 1) u times the sum of magnitudes, and u = 2^-23 also covers an adder that truncates; the 8 covers the chain
additions and the one fp32 multiply by s.  The gate is about 2^8 tighter than one wrong operand rounding, and where the
bound is 0 (column 2 of h, row 2 of d_wi, the all-zero row) it asks for exact zero.  Largest |err| / bound per tensor:
profiles/t5_bf16_error.txt.

Data: tests/test_gpu_t5_ffn.py:_data (one row scaled by 1e-3, one by 1e3, one all zero, row 2 of wi zero; everything in
bf16's normal range).  Shapes: (d, F) = (32, 32), (64, 96), (128, 256), (384, 1024); N = 1, 15, 16, 17, 31, 32, 33, 200;
p = 0, 0.1, 0.5; (32, 32) at N = 16401 (the 32-row tile) and (64, 64) at N = 1300 (several chains per wave in the weight
gradient)."""
import inspect

import pytest
import torch

from retrieval_cases import same_bits, seed as _seed
from test_gpu_t5_ffn import NS, PS, SHAPES, _data, _keep

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
BF = "bf16"


def bf(t):
    """The bf16 rounding (nearest even) of an fp32 tensor, as fp64."""
    return t.to(torch.bfloat16).to(torch.float64)


def gate(name, got, ref, mag, K):
    """The elementwise gate |got - ref| <= (K + 8) u mag; prints and returns the largest |err| / bound."""
    assert torch.isfinite(got).all(), name
    bound = (K + 8) * U * mag
    err = (got.double() - ref).abs()
    ratio = float((err / bound)[bound > 0].max()) if bool((bound > 0).any()) else 0.0
    print(f"ratio {name}: {ratio:.4f}")
    bad = err > bound
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} elements beyond the bound, largest ratio {ratio:.3f}; first {i}: "
                             f"kernel {float(got[i])!r}, fp64 {float(ref[i])!r}, |err| {float(err[i]):.6e}, bound "
                             f"{float(bound[i]):.6e} (row {i[0]} of a, column {i[1]} of b are its terms)")
    return ratio


def check(name, got, a, b, K, scale=1.0, where=None):
    """gate of `got` against scale * (a @ b) in fp64, zero outside `where`."""
    ref, mag = (a @ b) * scale, (a.abs() @ b.abs()) * abs(scale)
    if where is not None:
        ref, mag = torch.where(where, ref, torch.zeros_like(ref)), torch.where(where, mag, torch.zeros_like(mag))
    return gate(name, got, ref, mag, K)


def case(N, d, F, p, ordinary=False, tag=""):
    """Forward and backward of one shape in the "bf16" arithmetic: every gate -> (y, h, g, d_x, d_wi, d_wo)."""
    from rqhip import ops
    name = f"{tag}d={d} F={F} N={N} p={p}"
    x, wi, wo, d_y = _data(N, d, F, ordinary)
    seed = _seed(17 * N + d + F)
    keep = _keep(seed, N, F, p)
    s = 1.0 / (1.0 - p)
    with torch.no_grad():
        y, h = ops.t5_ffn_fwd(x, wi, wo, p, seed, arith=BF)
        d_x, d_wi, d_wo, g = ops.t5_ffn_bwd(x, wi, wo, h, d_y, p, seed, return_g=True, arith=BF)
        # hd as the kernels form it: one fp32 multiply by (float)s of the kernel's own h
        hd = h if keep is None else torch.where(keep, h * s, torch.zeros_like(h))
        s32 = float(torch.tensor(s, dtype=torch.float32)) if p > 0 else 1.0
    assert y.shape == (N, d) and h.shape == (N, F) and g.shape == (N, F)
    assert d_x.shape == (N, d) and d_wi.shape == (F, d) and d_wo.shape == (d, F)
    bx, bwi, bwo, bdy, bhd, bg = bf(x), bf(wi), bf(wo), bf(d_y), bf(hd), bf(g)
    # relu contracts: |relu(u) - relu(v)| <= |u - v|
    gate(f"{name} h", h, torch.relu(bx @ bwi.t()), bx.abs() @ bwi.abs().t(), d)
    assert not bool((h.view(torch.int32) == -2 ** 31).any()), name          # -0 never appears in h
    assert not bool(h.view(torch.int32)[:, 2].any()), name                   # the zero row of wi: exactly +0
    on = h > 0 if keep is None else (h > 0) & keep
    check(f"{name} y", y, bhd, bwo.t(), F)
    check(f"{name} g", g, bdy, bwo, d, scale=s32, where=on)
    check(f"{name} d_x", d_x, bg, bwi, F)
    check(f"{name} d_wi", d_wi, bg.t(), bx, N)
    check(f"{name} d_wo", d_wo, bdy.t(), bhd, N)
    assert not bool(d_wi[2].any()), name
    if N >= 4 and not ordinary:                                              # the all-zero row of x
        assert not bool(h[3].any()) and not bool(y[3].any()) and not bool(g[3].any()) and not bool(d_x[3].any()), name
    return y, h, g, d_x, d_wi, d_wo


@pytest.mark.parametrize("d,F", SHAPES)
def test_forward_and_backward(d, F):
    from rqhip import ops
    for N in NS:
        x, wi, wo, _ = _data(N, d, F)
        with torch.no_grad():
            plain = ops.t5_ffn_fwd(x, wi, wo, arith=BF)
        for p in PS:
            y, h, *_ = case(N, d, F, p)
            assert same_bits(h, plain[1]), (N, p)             # h does not know about the dropout
            if p == 0:
                assert same_bits(y, plain[0]), N              # p = 0 with and without a seed


@pytest.mark.parametrize("d,F,N", [(32, 32, 16401), (64, 64, 1300)])
def test_tall_tile_and_several_chains_per_wave(d, F, N):
    for p in (0.0, 0.1):
        case(N, d, F, p)
        case(N, d, F, p, ordinary=True, tag="ordinary ")


@pytest.mark.parametrize("d,F", SHAPES)
def test_same_bits_twice_and_rows_do_not_depend_on_the_batch(d, F):
    from rqhip import ops
    x, wi, wo, d_y = _data(200, d, F)

    def run(p, seed, n):
        with torch.no_grad():
            y, h = ops.t5_ffn_fwd(x[:n], wi, wo, p, seed, arith=BF)
            d_x, d_wi, d_wo, g = ops.t5_ffn_bwd(x[:n], wi, wo, h, d_y[:n], p, seed, return_g=True, arith=BF)
        return h, y, g, d_x, d_wi, d_wo

    for p in PS:
        a, b = run(p, _seed(3), 200), run(p, _seed(3), 200)
        assert all(same_bits(u, v) for u, v in zip(a, b)), p
        short = run(p, _seed(3), 17)                # the mask is a function of (row, column): the same on these rows
        for k, nm in enumerate(("h", "y", "g", "d_x")):
            assert same_bits(a[k][:17], short[k]), (p, nm)


def test_unwanted_outputs_leave_the_others_unchanged():
    from rqhip import ops
    N, d, F = 33, 64, 96
    x, wi, wo, d_y = _data(N, d, F)
    seed = _seed(5)
    with torch.no_grad():
        y, h = ops.t5_ffn_fwd(x, wi, wo, 0.1, seed, arith=BF)
        y2, none = ops.t5_ffn_fwd(x, wi, wo, 0.1, seed, need_h=False, arith=BF)
        assert none is None and same_bits(y, y2)
        full = ops.t5_ffn_bwd(x, wi, wo, h, d_y, 0.1, seed, arith=BF)
        assert len(full) == 3
        for need in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (0, 0, 0)):
            got = ops.t5_ffn_bwd(x, wi, wo, h, d_y, 0.1, seed, need_x=bool(need[0]), need_wi=bool(need[1]),
                                 need_wo=bool(need[2]), return_g=True, arith=BF)
            assert (got[3] is not None) == bool(need[1]), need      # g is the workspace of d_wi
            for n, a, b in zip(need, got, full):
                assert (a is None and not n) or (n and same_bits(a, b)), need


def test_function_matches_the_direct_calls():
    from rqhip import ops
    from rqhip.autograd import T5FFNFunction
    assert ops.T5_BF16 == (BF, False, False) and ops.T5_FP32 == ("fp32", False, False)
    assert inspect.signature(T5FFNFunction.forward).parameters["form"].default is ops.T5_FP32
    R, L, d, F = 5, 13, 64, 96
    x, wi, wo, d_y = _data(R * L, d, F)
    seed = _seed(9)
    for p in (0.0, 0.1):
        with torch.no_grad():
            y, h = ops.t5_ffn_fwd(x, wi, wo, p, seed, arith=BF)
            g = ops.t5_ffn_bwd(x, wi, wo, h, d_y, p, seed, arith=BF)
            y32, _ = ops.t5_ffn_fwd(x, wi, wo, p, seed)
        assert not same_bits(y, y32)
        xs, wis, wos = (t.clone().requires_grad_() for t in (x.view(R, L, d), wi, wo))
        out = T5FFNFunction.apply(xs, wis, wos, p, seed, ops.T5_BF16)
        assert same_bits(out.view(-1, d), y)
        out.backward(d_y.view(R, L, d))
        assert same_bits(xs.grad.view(-1, d), g[0]) and same_bits(wis.grad, g[1]) and same_bits(wos.grad, g[2])
        assert same_bits(T5FFNFunction.apply(x, wi, wo, p, seed), y32)       # the fp32 arm is where it was


@pytest.mark.parametrize("d,F", SHAPES)
def test_sanity_against_fp32(d, F):
    """A cap against a wildly wrong result, not an accuracy claim: on ordinary rows max|y_bf16 - y_fp32| / max|y_fp32| is
    below 2^-6, four times bf16's unit roundoff."""
    from rqhip import ops
    x, wi, wo, _ = _data(200, d, F, ordinary=True)
    with torch.no_grad():
        y16 = ops.t5_ffn_fwd(x, wi, wo, arith=BF)[0]
        y32 = ops.t5_ffn_fwd(x, wi, wo)[0]
    rel = float((y16 - y32).abs().max() / y32.abs().max())
    print(f"sanity d={d} F={F}: max|y_bf16 - y_fp32| / max|y_fp32| = {rel:.3e}")
    assert 0 < rel < 2.0 ** -6
