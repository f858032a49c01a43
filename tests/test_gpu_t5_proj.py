"""The grouped linear maps on the GPU: ops.t5_proj_fwd / ops.t5_proj_bwd (csrc/t5_proj.hip) against x @ w.t() and
autograd on the same inputs.

Gates (retrieval_cases.gate): e = max|a - a64| / max|a64| per tensor, for the kernel and for the operators in fp32 on
the same inputs, both against the operators in fp64 (under autograd for the gradients); e_kernel <= max(4 e_torch,
2^-22) for every y[j], e_kernel <= max(8 e_torch, 2^-22) for d_x and every d_w[j].  A tensor whose fp64 reference is
exactly zero must be exactly zero.  Measured ratios: profiles/t5_proj_error.txt.

Shapes: (d_in, d_out) = (32, 32) (one group, a quarter chunk), (64, 96) (a partial chain; a partial chunk with idle
waves at n = 1), (384, 384) (the model's: three chains, nine chunks at n = 3), (512, 64) (the longest reduction, the
chain of d_x across the weights of the group).  n = 1, 2, 3, 8.  N = 1, 15 / 16 / 17 (the 16-row tile), 31 / 32 / 33
(the weight gradient's 32-row block), 200 (a partial last block, unequal block ranges of the four waves), 1300 rows
at (64, 64) (waves with more than 8 blocks: several chains per wave), and 8209 and 16401 rows at the two small shapes
(the 32-row and the 64-row tile of long batches, 17 rows in their last tile).  Rows: normal, one scaled by 1e-3, one by 1e3,
one all zero in x, one all zero in every d_y; row 2 of weight 0 is zero, so column 2 of y[0] is exactly +0.  With the
1e3 row in a case it sets max|a64| of every tensor, so test_ordinary_rows_alone repeats the gates on normal rows only."""
import pytest
import torch

from retrieval_cases import gate, same_bits

pytestmark = pytest.mark.gpu

SHAPES = ((32, 32), (64, 96), (384, 384), (512, 64))
GROUPS = (1, 2, 3, 8)
NS = (1, 15, 16, 17, 31, 32, 33, 200)


def _data(N, d_in, d_out, n, ordinary=False):
    g = torch.Generator().manual_seed(100000 * d_in + 100 * d_out + 10 * n + N % 97)
    x = torch.randn(N, d_in, generator=g)
    d_ys = [torch.randn(N, d_out, generator=g) for _ in range(n)]
    ws = [torch.randn(d_out, d_in, generator=g) * d_in ** -0.5 for _ in range(n)]
    if not ordinary:
        for t in [x] + d_ys:
            if N >= 3:
                t[1] *= 1e-3
                t[2] *= 1e3
        if N >= 4:
            x[3] = 0
        if N >= 5:
            for t in d_ys:
                t[4] = 0
    ws[0][2] = 0
    dev = torch.device("cuda")
    return x.to(dev), [w.to(dev) for w in ws], [t.to(dev) for t in d_ys]


def _chain(x, ws, d_ys, dtype):
    """The operators in `dtype` -> (ys, d_x, d_ws)."""
    x = x.detach().to(dtype).requires_grad_()
    ws = [w.detach().to(dtype).requires_grad_() for w in ws]
    ys = [x @ w.t() for w in ws]
    grads = torch.autograd.grad(ys, [x] + ws, [t.to(dtype) for t in d_ys])
    return [y.detach() for y in ys], grads[0], list(grads[1:])


def _case(N, d_in, d_out, n, ordinary=False, tag=""):
    from rqhip import ops
    name = f"{tag}d_in={d_in} d_out={d_out} n={n} N={N}"
    x, ws, d_ys = _data(N, d_in, d_out, n, ordinary)
    with torch.no_grad():
        ys = ops.t5_proj_fwd(x, ws)
        d_x, d_ws = ops.t5_proj_bwd(x, ws, d_ys)
    assert len(ys) == n and len(d_ws) == n and d_x.shape == (N, d_in)
    assert all(y.shape == (N, d_out) for y in ys) and all(g.shape == (d_out, d_in) for g in d_ws)
    ys64, d_x64, d_ws64 = _chain(x, ws, d_ys, torch.float64)
    ys32, d_x32, d_ws32 = _chain(x, ws, d_ys, torch.float32)
    for j in range(n):
        gate(f"{name} y[{j}]", ys[j], ys32[j], ys64[j], 4)
    gate(f"{name} d_x", d_x, d_x32, d_x64, 8)
    for j in range(n):
        gate(f"{name} d_w[{j}]", d_ws[j], d_ws32[j], d_ws64[j], 8)
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
            _case(N, d_in, d_out, n)


@pytest.mark.parametrize("d_in,d_out", SHAPES)
def test_ordinary_rows_alone(d_in, d_out):
    """The same gates with no scaled and no all-zero row, so no single row hides the others behind max|a64|."""
    for n in GROUPS:
        for N in (17, 33, 200):
            _case(N, d_in, d_out, n, ordinary=True, tag="ordinary ")


def test_long_reduction_over_the_rows():
    for n in (1, 3):
        _case(1300, 64, 64, n)
        _case(1300, 64, 64, n, ordinary=True, tag="ordinary ")


@pytest.mark.parametrize("N", [8209, 16401])
def test_taller_row_tiles_of_long_batches(N):
    """Above 8192 rows a row tile is 32 rows high, above 16384 rows 64 (17 rows in the last tile here): the same gates,
    and a row's bits are those of the one-row call, which a 16-row tile computes."""
    from rqhip import ops
    for d_in, d_out, n in ((32, 32, 1), (64, 96, 3)):
        ys, d_x, _ = _case(N, d_in, d_out, n)
        _case(N, d_in, d_out, n, ordinary=True, tag="ordinary ")
        x, ws, d_ys = _data(N, d_in, d_out, n)
        with torch.no_grad():
            for r in (0, 1, 15, 16, 31, 32, 63, 64, 8191, 8192, N - 17, N - 1):
                one = ops.t5_proj_fwd(x[r:r + 1], ws)
                one_x = ops.t5_proj_bwd(x[r:r + 1], ws, [t[r:r + 1] for t in d_ys], need_w=[False] * n)[0]
                assert all(same_bits(a, b[r:r + 1]) for a, b in zip(one, ys)) and same_bits(one_x, d_x[r:r + 1]), r


@pytest.mark.parametrize("d_in,d_out", SHAPES)
def test_same_bits_in_every_group_at_every_batch_and_twice(d_in, d_out):
    from rqhip import ops
    N = 200
    x, ws, d_ys = _data(N, d_in, d_out, 8)
    with torch.no_grad():
        ys, (d_x, d_ws) = ops.t5_proj_fwd(x, ws), ops.t5_proj_bwd(x, ws, d_ys)
        # a second run of every call
        ys2, (d_x2, d_ws2) = ops.t5_proj_fwd(x, ws), ops.t5_proj_bwd(x, ws, d_ys)
        assert all(same_bits(a, b) for a, b in zip(ys + (d_x,) + tuple(d_ws), ys2 + (d_x2,) + tuple(d_ws2)))
        # y[j] knows neither n nor the other weights of its group; d_w[j] neither
        three = ops.t5_proj_fwd(x, ws[2:5])
        g3_x, g3_w = ops.t5_proj_bwd(x, ws[2:5], d_ys[2:5])
        three_again = ops.t5_proj_fwd(x, ws[2:5])
        assert all(same_bits(a, b) for a, b in zip(three, three_again))
        for j in range(8):
            one = ops.t5_proj_fwd(x, [ws[j]])[0]
            assert same_bits(one, ys[j]), j
            if 2 <= j < 5:
                assert same_bits(one, three[j - 2]) and same_bits(g3_w[j - 2], d_ws[j]), j
        # a row's y and d_x are the same at N = 17 and N = 200, wherever the row stands
        short = ops.t5_proj_fwd(x[:17], ws[2:5])
        short_x = ops.t5_proj_bwd(x[:17], ws[2:5], [t[:17] for t in d_ys[2:5]], need_w=[False] * 3)[0]
        assert all(same_bits(a, b[:17]) for a, b in zip(short, three)) and same_bits(short_x, g3_x[:17])
        moved = ops.t5_proj_fwd(x[150:167], ws[2:5])
        moved_x = ops.t5_proj_bwd(x[150:167], ws[2:5], [t[150:167] for t in d_ys[2:5]], need_w=[False] * 3)[0]
        assert all(same_bits(a, b[150:167]) for a, b in zip(moved, three)) and same_bits(moved_x, g3_x[150:167])
        for r in (0, 15, 16, N - 1):
            assert same_bits(ops.t5_proj_fwd(x[r:r + 1], [ws[0]])[0], ys[0][r:r + 1]), r


@pytest.mark.parametrize("d_in,d_out", SHAPES)
def test_missing_upstream_gradients_and_unwanted_outputs(d_in, d_out):
    from rqhip import ops
    N = 33
    x, ws, d_ys = _data(N, d_in, d_out, 3)
    with torch.no_grad():
        full_x, full_w = ops.t5_proj_bwd(x, ws, d_ys)
        # d_y[1] missing: the call on the remaining group, and no d_w[1]
        rest_x, rest_w = ops.t5_proj_bwd(x, [ws[0], ws[2]], [d_ys[0], d_ys[2]])
        got_x, got_w = ops.t5_proj_bwd(x, ws, [d_ys[0], None, d_ys[2]])
        assert same_bits(got_x, rest_x) and got_w[1] is None
        assert same_bits(got_w[0], rest_w[0]) and same_bits(got_w[2], rest_w[1])
        assert same_bits(got_w[0], full_w[0]) and same_bits(got_w[2], full_w[2])
        # no upstream gradient at all
        none_x, none_w = ops.t5_proj_bwd(x, ws, [None, None, None])
        assert none_x is None and none_w == [None, None, None]
        # each choice of wanted gradients leaves the others' bits alone
        for need_x in (True, False):
            for need_w in ([True, False, True], [False, False, False], [False, True, False]):
                g_x, g_w = ops.t5_proj_bwd(x, ws, d_ys, need_x=need_x, need_w=need_w)
                assert (g_x is None and not need_x) or same_bits(g_x, full_x)
                for f, a, b in zip(need_w, g_w, full_w):
                    assert (a is None and not f) or (f and same_bits(a, b))


@pytest.mark.parametrize("N", [17, 33])
def test_row_strided_outputs_leave_their_surroundings_untouched(N):
    """Outputs written through a row stride larger than d_out (a position of a decode-cache slab among them): the guard
    columns and the rows past N keep their sentinel."""
    from rqhip import ops
    d_in, d_out, pad, extra = 64, 96, 8, 3
    x, ws, _ = _data(N, d_in, d_out, 3)
    sentinel = -7.25
    with torch.no_grad():
        dense = ops.t5_proj_fwd(x, ws)
        bufs = [torch.full((N + extra, d_out + pad), sentinel, device=x.device) for _ in range(2)]
        slab = torch.full((4, N + extra, d_out), sentinel, device=x.device)
        outs = ops.t5_proj_fwd(x.view(N, 1, d_in), ws, [None, bufs[1][:N, :d_out], slab[2, :N]])
    assert outs[0].shape == (N, 1, d_out) and same_bits(outs[0].view(N, d_out), dense[0])
    assert outs[1].data_ptr() == bufs[1].data_ptr() and outs[2].data_ptr() == slab[2].data_ptr()
    assert same_bits(bufs[1][:N, :d_out], dense[1]) and same_bits(slab[2, :N], dense[2])
    assert bool((bufs[1][:, d_out:] == sentinel).all()) and bool((bufs[1][N:] == sentinel).all())
    assert bool((slab[2, N:] == sentinel).all()) and bool((slab[[0, 1, 3]] == sentinel).all())
    assert bool((bufs[0] == sentinel).all())


def test_function_matches_the_direct_calls():
    from rqhip import ops
    from rqhip.autograd import T5ProjFunction
    R, L, d_in, d_out = 5, 13, 64, 96
    x, ws, d_ys = _data(R * L, d_in, d_out, 3)
    with torch.no_grad():
        ys = ops.t5_proj_fwd(x, ws)
        g_x, g_w = ops.t5_proj_bwd(x, ws, d_ys)
        h_x, h_w = ops.t5_proj_bwd(x, ws, [d_ys[0], None, d_ys[2]])
    xs = x.view(R, L, d_in).clone().requires_grad_()
    wss = [w.clone().requires_grad_() for w in ws]
    outs = T5ProjFunction.apply(xs, ops.T5_FP32, *wss)
    assert len(outs) == 3 and all(o.shape == (R, L, d_out) and same_bits(o.view(-1, d_out), y) for o, y in zip(outs, ys))
    d_nc = d_ys[0].view(R, L, d_out).transpose(0, 1).contiguous().transpose(0, 1)       # non-contiguous upstream gradient
    assert not d_nc.is_contiguous()
    torch.autograd.backward(outs, [d_nc, d_ys[1].view(R, L, d_out), d_ys[2].view(R, L, d_out)])
    assert same_bits(xs.grad.view(-1, d_in), g_x) and all(same_bits(w.grad, g) for w, g in zip(wss, g_w))
    # an output nobody used: no gradient for its weight, and it is left out of d_x
    xs = x.clone().requires_grad_()
    wss = [w.clone().requires_grad_() for w in ws]
    outs = T5ProjFunction.apply(xs, ops.T5_FP32, *wss)
    torch.autograd.backward([outs[0], outs[2]], [d_ys[0], d_ys[2]])
    assert same_bits(xs.grad, h_x) and wss[1].grad is None
    assert same_bits(wss[0].grad, h_w[0]) and same_bits(wss[2].grad, h_w[2])
    # only the input needs a gradient: frozen weights
    xs = x.clone().requires_grad_()
    torch.autograd.backward(T5ProjFunction.apply(xs, ops.T5_FP32, *ws), d_ys)
    assert same_bits(xs.grad, g_x)
    # only some weights do
    w1 = ws[1].clone().requires_grad_()
    torch.autograd.backward(T5ProjFunction.apply(x, ops.T5_FP32, ws[0], w1, ws[2]), d_ys)
    assert same_bits(w1.grad, g_w[1])


def test_views_off_a_16_byte_boundary_are_realigned():
    from rqhip import ops
    N, d_in, d_out = 17, 64, 96
    x, ws, d_ys = _data(N, d_in, d_out, 2)

    def off(t):
        buf = torch.empty(t.numel() + 1, device=t.device)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v

    with torch.no_grad():
        want = ops.t5_proj_fwd(x, ws)
        got = ops.t5_proj_fwd(off(x), [off(w) for w in ws])
        assert all(same_bits(a, b) for a, b in zip(want, got))
        want_x, want_w = ops.t5_proj_bwd(x, ws, d_ys)
        got_x, got_w = ops.t5_proj_bwd(off(x), [off(w) for w in ws], [off(t) for t in d_ys])
        assert same_bits(want_x, got_x) and all(same_bits(a, b) for a, b in zip(want_w, got_w))
        # an output that starts off a 16-byte boundary is written where it is
        out = off(torch.zeros(N, d_out, device=x.device))
        assert ops.t5_proj_fwd(x, ws, [out, None])[0] is out and same_bits(out, want[0])


def test_wrappers_reject_what_the_kernel_does_not_take():
    from rqhip import ops
    from rqhip._lib import RqHipError
    dev = torch.device("cuda")
    x, w = torch.zeros(3, 32, device=dev), torch.zeros(64, 32, device=dev)
    with pytest.raises(RqHipError, match="float32"):
        ops.t5_proj_fwd(x.half(), [w.half()])
    with pytest.raises(RqHipError, match=r"weights\[1\] must be"):
        ops.t5_proj_fwd(x, [w, torch.zeros(32, 32, device=dev)])
    with pytest.raises(RqHipError, match="not supported"):
        ops.t5_proj_fwd(x, [w] * 9)
    with pytest.raises(RqHipError, match="not supported"):
        ops.t5_proj_fwd(x, [])
    with pytest.raises(RqHipError, match="not supported"):
        ops.t5_proj_fwd(torch.zeros(3, 48, device=dev), [torch.zeros(64, 48, device=dev)])
    with pytest.raises(RqHipError, match=r"outs\[0\] must be"):
        ops.t5_proj_fwd(x, [w], [torch.zeros(3, 128, device=dev)[:, ::2]])
    with pytest.raises(RqHipError, match=r"outs\[0\] must be"):
        ops.t5_proj_fwd(x, [w], [torch.zeros(2, 64, device=dev)])
    with pytest.raises(RqHipError, match="1 outs for 2 weights"):
        ops.t5_proj_fwd(x, [w, w], [None])
    with pytest.raises(RqHipError, match="does not match"):
        ops.t5_proj_bwd(x, [w], [torch.zeros(2, 64, device=dev)])
    with pytest.raises(RqHipError, match="2 d_ys"):
        ops.t5_proj_bwd(x, [w], [None, None])
    # no rows: nothing is launched, the weight gradients are empty sums
    e = torch.zeros(0, 32, device=dev)
    (y,) = ops.t5_proj_fwd(e, [w])
    assert y.shape == (0, 64)
    d_x, d_w = ops.t5_proj_bwd(e, [w], [y])
    assert d_x.shape == (0, 32) and d_w[0].shape == (64, 32) and not bool(d_w[0].any())
    (y,) = ops.t5_proj_fwd(torch.zeros(2, 0, 32, device=dev), [w])
    assert y.shape == (2, 0, 64)
