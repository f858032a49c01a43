"""The "bf16" arithmetic of the grouped linear maps on the GPU: ops.t5_proj_fwd / ops.t5_proj_bwd with arith="bf16"
(csrc/t5_proj.hip, rqhip_t5_proj_*_bf16) against fp64 on operands rounded to bf16 on the host.

Gate (tests/test_gpu_t5_ffn_bf16.py:check, derived there), elementwise: |kernel - ref64| <= (K + 8) * 2^-23 * (|a| @ |b|)
  y[j]    against bf(x) @ bf(w[j]).T, K = d_in
  d_x     against the product over the concatenation of the live (j, term) pairs, K = its length, live * d_out
  d_w[j]  against bf(d_y[j]).T @ bf(x), K = N
Where the bound is 0 (column 2 of y[0], the all-zero rows) exact zero is required.  Largest |err| / bound per tensor:
profiles/t5_bf16_error.txt.

Data, shapes, group sizes and strides: tests/test_gpu_t5_proj.py's.  N = 16401 runs the 64-row tile."""
import pytest
import torch

from retrieval_cases import same_bits
from test_gpu_t5_ffn_bf16 import bf, check
from test_gpu_t5_proj import GROUPS, NS, SHAPES, _data

pytestmark = pytest.mark.gpu

BF = "bf16"


def case(N, d_in, d_out, n, ordinary=False, tag="", missing=()):
    """Forward and backward of one group in the "bf16" arithmetic, the d_ys[j] of `missing` None: every gate."""
    from rqhip import ops
    name = f"{tag}d_in={d_in} d_out={d_out} n={n} N={N}" + (f" without {list(missing)}" if missing else "")
    x, ws, d_ys = _data(N, d_in, d_out, n, ordinary)
    given = [None if j in missing else t for j, t in enumerate(d_ys)]
    with torch.no_grad():
        ys = ops.t5_proj_fwd(x, ws, arith=BF)
        d_x, d_ws = ops.t5_proj_bwd(x, ws, given, arith=BF)
    assert len(ys) == n and len(d_ws) == n and d_x.shape == (N, d_in)
    bx, bws = bf(x), [bf(w) for w in ws]
    for j in range(n):
        check(f"{name} y[{j}]", ys[j], bx, bws[j].t(), d_in)
    live = [j for j in range(n) if j not in missing]
    check(f"{name} d_x", d_x, torch.cat([bf(d_ys[j]) for j in live], dim=1), torch.cat([bws[j] for j in live], dim=0),
          len(live) * d_out)
    for j in range(n):
        if j in missing:
            assert d_ws[j] is None, name
        else:
            check(f"{name} d_w[{j}]", d_ws[j], bf(d_ys[j]).t(), bx, N)
    assert not bool(ys[0][:, 2].any()), name                     # the zero row of weight 0
    if N >= 4 and not ordinary:                                  # the all-zero row of x
        assert not any(bool(y[3].any()) for y in ys), name
    if N >= 5 and not ordinary:                                  # the all-zero row of every d_y
        assert not bool(d_x[4].any()), name
    return ys, d_x, d_ws


@pytest.mark.parametrize("d_in,d_out", SHAPES)
def test_forward_and_backward(d_in, d_out):
    for n in GROUPS:
        for N in NS:
            case(N, d_in, d_out, n)
    case(33, d_in, d_out, 3, missing=(1,))
    case(200, d_in, d_out, 8, ordinary=True, tag="ordinary ", missing=(0, 5))


def test_long_reduction_over_the_rows():
    for n in (1, 3):
        case(1300, 64, 64, n)
        case(1300, 64, 64, n, ordinary=True, tag="ordinary ")


def test_the_64_row_tile():
    """Above 16384 rows a row tile is 64 rows high (17 rows in the last tile here): the same gates, and a row's bits are
    those of the one-row call, which a 16-row tile computes."""
    from rqhip import ops
    N = 16401
    for d_in, d_out, n in ((32, 32, 1), (64, 96, 3)):
        ys, d_x, _ = case(N, d_in, d_out, n)
        x, ws, d_ys = _data(N, d_in, d_out, n)
        with torch.no_grad():
            for r in (0, 15, 16, 63, 64, 16383, 16384, N - 1):
                one = ops.t5_proj_fwd(x[r:r + 1], ws, arith=BF)
                one_x = ops.t5_proj_bwd(x[r:r + 1], ws, [t[r:r + 1] for t in d_ys], need_w=[False] * n, arith=BF)[0]
                assert all(same_bits(a, b[r:r + 1]) for a, b in zip(one, ys)) and same_bits(one_x, d_x[r:r + 1]), r


@pytest.mark.parametrize("d_in,d_out", SHAPES)
def test_same_bits_in_every_group_at_every_batch_and_twice(d_in, d_out):
    from rqhip import ops
    N = 200
    x, ws, d_ys = _data(N, d_in, d_out, 8)
    with torch.no_grad():
        ys, (d_x, d_ws) = ops.t5_proj_fwd(x, ws, arith=BF), ops.t5_proj_bwd(x, ws, d_ys, arith=BF)
        ys2, (d_x2, d_ws2) = ops.t5_proj_fwd(x, ws, arith=BF), ops.t5_proj_bwd(x, ws, d_ys, arith=BF)
        assert all(same_bits(a, b) for a, b in zip(ys + (d_x,) + tuple(d_ws), ys2 + (d_x2,) + tuple(d_ws2)))
        assert not same_bits(ys[1], ops.t5_proj_fwd(x, [ws[1]])[0])        # it is another arithmetic than fp32
        # y[j] knows neither n nor the other weights of its group; d_w[j] neither
        three = ops.t5_proj_fwd(x, ws[2:5], arith=BF)
        g3_x, g3_w = ops.t5_proj_bwd(x, ws[2:5], d_ys[2:5], arith=BF)
        for j in range(8):
            one = ops.t5_proj_fwd(x, [ws[j]], arith=BF)[0]
            assert same_bits(one, ys[j]), j
            if 2 <= j < 5:
                assert same_bits(one, three[j - 2]) and same_bits(g3_w[j - 2], d_ws[j]), j
        # a row's y and d_x are the same at N = 17 and N = 200, wherever the row stands
        for rows in (slice(0, 17), slice(150, 167)):
            part = ops.t5_proj_fwd(x[rows], ws[2:5], arith=BF)
            part_x = ops.t5_proj_bwd(x[rows], ws[2:5], [t[rows] for t in d_ys[2:5]], need_w=[False] * 3, arith=BF)[0]
            assert all(same_bits(a, b[rows]) for a, b in zip(part, three)) and same_bits(part_x, g3_x[rows])
        # d_x with a None equals the call on the remaining group, and that d_w[j] is not produced
        rest_x, rest_w = ops.t5_proj_bwd(x, [ws[2], ws[4]], [d_ys[2], d_ys[4]], arith=BF)
        got_x, got_w = ops.t5_proj_bwd(x, ws[2:5], [d_ys[2], None, d_ys[4]], arith=BF)
        assert same_bits(got_x, rest_x) and got_w[1] is None
        assert same_bits(got_w[0], rest_w[0]) and same_bits(got_w[2], rest_w[1])


@pytest.mark.parametrize("N", [17, 33])
def test_strided_inputs_and_outputs(N):
    """x as a view with a row stride, outputs written through a row stride larger than d_out (a position of a
    decode-cache slab among them): the dense call's bits, and the guard columns and the rows past N keep their sentinel."""
    from rqhip import ops
    d_in, d_out, pad, extra = 64, 96, 8, 3
    x, ws, _ = _data(N, d_in, d_out, 3)
    sentinel = -7.25
    with torch.no_grad():
        dense = ops.t5_proj_fwd(x, ws, arith=BF)
        wide = torch.full((N, d_in + pad), sentinel, device=x.device)
        wide[:, :d_in] = x
        assert all(same_bits(a, b) for a, b in zip(ops.t5_proj_fwd(wide[:, :d_in], ws, arith=BF), dense))
        bufs = [torch.full((N + extra, d_out + pad), sentinel, device=x.device) for _ in range(2)]
        slab = torch.full((4, N + extra, d_out), sentinel, device=x.device)
        outs = ops.t5_proj_fwd(x.view(N, 1, d_in), ws, [None, bufs[1][:N, :d_out], slab[2, :N]], arith=BF)
    assert outs[0].shape == (N, 1, d_out) and same_bits(outs[0].view(N, d_out), dense[0])
    assert outs[1].data_ptr() == bufs[1].data_ptr() and outs[2].data_ptr() == slab[2].data_ptr()
    assert same_bits(bufs[1][:N, :d_out], dense[1]) and same_bits(slab[2, :N], dense[2])
    assert bool((bufs[1][:, d_out:] == sentinel).all()) and bool((bufs[1][N:] == sentinel).all())
    assert bool((slab[2, N:] == sentinel).all()) and bool((slab[[0, 1, 3]] == sentinel).all())
    assert bool((bufs[0] == sentinel).all())


def test_function_matches_the_direct_calls():
    from rqhip import ops
    from rqhip.autograd import T5ProjFunction
    assert ops.T5_BF16 == (BF, False, False) and ops.T5_FP32 == ("fp32", False, False)
    R, L, d_in, d_out = 5, 13, 64, 96
    x, ws, d_ys = _data(R * L, d_in, d_out, 3)
    with torch.no_grad():
        ys = ops.t5_proj_fwd(x, ws, arith=BF)
        g_x, g_w = ops.t5_proj_bwd(x, ws, d_ys, arith=BF)
        h_x, h_w = ops.t5_proj_bwd(x, ws, [d_ys[0], None, d_ys[2]], arith=BF)
    xs = x.view(R, L, d_in).clone().requires_grad_()
    wss = [w.clone().requires_grad_() for w in ws]
    outs = T5ProjFunction.apply(xs, ops.T5_BF16, *wss)
    assert len(outs) == 3 and all(same_bits(o.view(-1, d_out), y) for o, y in zip(outs, ys))
    torch.autograd.backward(outs, [t.view(R, L, d_out) for t in d_ys])
    assert same_bits(xs.grad.view(-1, d_in), g_x) and all(same_bits(w.grad, g) for w, g in zip(wss, g_w))
    # an output nobody used: no gradient for its weight, and it is left out of d_x
    xs = x.clone().requires_grad_()
    wss = [w.clone().requires_grad_() for w in ws]
    outs = T5ProjFunction.apply(xs, ops.T5_BF16, *wss)
    torch.autograd.backward([outs[0], outs[2]], [d_ys[0], d_ys[2]])
    assert same_bits(xs.grad, h_x) and wss[1].grad is None
    assert same_bits(wss[0].grad, h_w[0]) and same_bits(wss[2].grad, h_w[2])
