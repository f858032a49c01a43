"""The fused T5 feed-forward on the GPU: ops.t5_ffn_fwd / ops.t5_ffn_bwd (csrc/t5_ffn.hip) against the operators of
modules/t5.py:T5DenseReluDense (wi, relu, dropout, wo) with the kernel's dropout mask inserted.

Gates (retrieval_cases.gate): e = max|a - a64| / max|a64| per tensor, for the kernel and for the operator chain in
fp32 on the same inputs, both against the chain in fp64 (under autograd for the gradients); e_kernel <= max(4 e_torch,
2^-22) for h and y, e_kernel <= max(8 e_torch, 2^-22) for d_x, d_wi and d_wo.  A tensor whose fp64 reference is exactly
zero must be exactly zero.  Measured ratios: profiles/t5_ffn_error.txt.

The backward is a function of (x, wi, wo, h, d_y): which units are active is read from the h it is given.  A
pre-activation within rounding of zero can fall on either side in fp32 and in fp64, and a gradient would then differ by
a whole term for a reason that is no error of the backward.  So the gradient chains take the active set from the
kernel's h (`act`), and the forward test checks that set against the fp64 pre-activation wherever that is not within
1e-5 of the largest one.

Shapes: (d, F) = (32, 32) (one column pair, a quarter chunk), (64, 96) (a partial chunk, idle waves), (128, 256) (two
chunks), (384, 1024) (the model's: three column pairs per wave), (512, 2048) (the largest widths in the model family).
N = 1, 15 / 16 / 17 / 33 (the 16-row tile), 31 / 32 / 33 (the weight gradient's 32-row block), 200 (a partial last
block, and unequal block ranges of the four waves), 16401 (the 32-row tile above 16384 rows, 17 rows in its last tile)
and 1300 rows at (64, 64) (waves with more than 8 blocks: several chains per wave).  Rows: normal, one scaled by 1e-3,
one by 1e3, one all zero; row 2 of wi is zero, so column 2 of h is exactly +0.  With the 1e3 row in a case it sets
max|a64| of every tensor, so test_ordinary_rows_alone repeats the gates on normal rows only."""
import pytest
import torch

from retrieval_cases import gate, same_bits, seed as _seed

pytestmark = pytest.mark.gpu

SHAPES = ((32, 32), (64, 96), (128, 256), (384, 1024))
NS = (1, 15, 16, 17, 31, 32, 33, 200)
PS = (0.0, 0.1, 0.5)
T = 16          # the row tile of every N <= 16384


def _data(N, d, F, ordinary=False):
    g = torch.Generator().manual_seed(100000 * d + 100 * F + N % 97)
    x, d_y = torch.randn(N, d, generator=g), torch.randn(N, d, generator=g)
    if N >= 3 and not ordinary:
        x[1] *= 1e-3
        d_y[1] *= 1e-3
        x[2] *= 1e3
        d_y[2] *= 1e3
    if N >= 4 and not ordinary:
        x[3] = 0
    wi = torch.randn(F, d, generator=g) * d ** -0.5
    wo = torch.randn(d, F, generator=g) * F ** -0.5
    wi[2] = 0
    dev = torch.device("cuda")
    return x.to(dev), wi.to(dev), wo.to(dev), d_y.to(dev)


def _keep(seed, N, F, p):
    from rqhip import ops
    return ops.t5_attention_dropout_keep(seed, 1, 1, N, F, p)[0, 0] if p > 0 else None


def _chain(x, wi, wo, keep, p, dtype, act=None, d_y=None):
    """The operators in `dtype` -> (pre, h, y, grads or None); `act`: the active set instead of pre > 0 (docstring)."""
    x, wi, wo = (t.detach().to(dtype).requires_grad_() for t in (x, wi, wo))
    pre = x @ wi.t()
    h = torch.relu(pre) if act is None else torch.where(act, pre, torch.zeros_like(pre))
    hd = h if keep is None else torch.where(keep, h * (1.0 / (1.0 - p)), torch.zeros_like(h))
    y = hd @ wo.t()
    grads = None
    if d_y is not None:
        grads = torch.autograd.grad([y], [x, wi, wo], [d_y.to(dtype)])
    return pre.detach(), h.detach(), y.detach(), grads


def _case(N, d, F, p, ordinary=False, tag=""):
    """Forward and backward of one shape: every gate, and what must hold bit for bit within one case."""
    from rqhip import ops
    name = f"{tag}d={d} F={F} N={N} p={p}"
    x, wi, wo, d_y = _data(N, d, F, ordinary)
    seed = _seed(17 * N + d + F)
    keep = _keep(seed, N, F, p)
    with torch.no_grad():
        y, h = ops.t5_ffn_fwd(x, wi, wo, p, seed)
        d_x, d_wi, d_wo = ops.t5_ffn_bwd(x, wi, wo, h, d_y, p, seed)
    assert y.shape == (N, d) and h.shape == (N, F) and d_x.shape == (N, d) and d_wi.shape == (F, d) and d_wo.shape == (d, F)
    pre64, h64, y64, _ = _chain(x, wi, wo, keep, p, torch.float64)
    _, h32, y32, _ = _chain(x, wi, wo, keep, p, torch.float32)
    gate(f"{name} h", h, h32, h64, 4)
    gate(f"{name} y", y, y32, y64, 4)
    # +0 wherever the pre-activation is <= 0, active wherever it is > 0 (rows apart in scale: compare within a row)
    clear = pre64.abs() > 1e-5 * pre64.abs().amax(dim=1, keepdim=True)
    act = h > 0
    assert torch.equal(act[clear], (pre64 > 0)[clear]), name
    assert not bool(h.view(torch.int32)[~act].any()), name          # +0, never -0
    assert not bool(h.view(torch.int32)[:, 2].any()), name          # the zero row of wi
    ref64 = _chain(x, wi, wo, keep, p, torch.float64, act, d_y)[3]
    ref32 = _chain(x, wi, wo, keep, p, torch.float32, act, d_y)[3]
    for nm, a, a32, a64 in zip(("d_x", "d_wi", "d_wo"), (d_x, d_wi, d_wo), ref32, ref64):
        gate(f"{name} {nm}", a, a32, a64, 8)
    assert not bool(d_wi[2].any()), name                            # g is 0 in that column
    if N >= 4 and not ordinary:                                     # the all-zero row of x
        assert not bool(h[3].any()) and not bool(y[3].any()) and not bool(d_x[3].any()), name
    return y, h, d_x, d_wi, d_wo


@pytest.mark.parametrize("d,F", SHAPES)
def test_forward_and_backward(d, F):
    from rqhip import ops
    for N in NS:
        x, wi, wo, _ = _data(N, d, F)
        with torch.no_grad():
            plain = ops.t5_ffn_fwd(x, wi, wo)
        for p in PS:
            y, h, *_ = _case(N, d, F, p)
            assert same_bits(h, plain[1]), (N, p)             # h does not know about the dropout
            if p == 0:
                assert same_bits(y, plain[0]), N              # p = 0 with and without a seed


@pytest.mark.parametrize("d,F", SHAPES)
def test_ordinary_rows_alone(d, F):
    """The same gates with no scaled and no all-zero row, so no single row hides the others behind max|a64|."""
    for N in (17, 33, 200):
        for p in PS:
            _case(N, d, F, p, ordinary=True, tag="ordinary ")


@pytest.mark.parametrize("d,F,N", [(512, 2048, 33), (64, 64, 1300), (32, 32, 16401), (64, 96, 16401)])
def test_largest_widths_long_reduction_and_tall_tile(d, F, N):
    for p in (0.0, 0.1):
        _case(N, d, F, p)
        _case(N, d, F, p, ordinary=True, tag="ordinary ")


@pytest.mark.parametrize("d,F", SHAPES)
def test_same_bits_twice_rows_alone_and_seeds(d, F):
    from rqhip import ops
    N = 200
    x, wi, wo, d_y = _data(N, d, F)

    def run(p, seed, rows=slice(None)):
        with torch.no_grad():
            y, h = ops.t5_ffn_fwd(x[rows], wi, wo, p, seed)
            return (y, h) + tuple(ops.t5_ffn_bwd(x[rows], wi, wo, h, d_y[rows], p, seed))

    for p in PS:
        a, b = run(p, _seed(3)), run(p, _seed(3))
        assert all(same_bits(u, v) for u, v in zip(a, b)), p
    whole = run(0.0, None)
    for r in (0, 1, T - 1, T, N - 1):
        one = run(0.0, None, slice(r, r + 1))
        for k in (0, 1, 2):          # y, h, d_x
            assert same_bits(whole[k][r:r + 1], one[k]), (r, k)
    a, b = run(0.5, _seed(3)), run(0.5, _seed(4))
    assert not same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    assert not same_bits(a[2], b[2]) and not same_bits(a[4], b[4])


def test_rows_of_the_tall_tile_do_not_depend_on_the_batch():
    """Above 16384 rows the tile is 32 rows high; a row's bits are those of the one-row call (a 16-row tile)."""
    from rqhip import ops
    N, d, F = 16401, 64, 96
    x, wi, wo, d_y = _data(N, d, F)
    with torch.no_grad():
        y, h = ops.t5_ffn_fwd(x, wi, wo)
        d_x = ops.t5_ffn_bwd(x, wi, wo, h, d_y, need_wi=False, need_wo=False)[0]
        for r in (0, 1, 31, 32, 16383, 16384, N - 1):
            y1, h1 = ops.t5_ffn_fwd(x[r:r + 1], wi, wo)
            d_x1 = ops.t5_ffn_bwd(x[r:r + 1], wi, wo, h1, d_y[r:r + 1], need_wi=False, need_wo=False)[0]
            assert same_bits(y[r:r + 1], y1) and same_bits(h[r:r + 1], h1) and same_bits(d_x[r:r + 1], d_x1), r


def test_unwanted_outputs_leave_the_others_unchanged():
    from rqhip import ops
    N, d, F = 33, 64, 96
    x, wi, wo, d_y = _data(N, d, F)
    seed = _seed(5)
    with torch.no_grad():
        y, h = ops.t5_ffn_fwd(x, wi, wo, 0.1, seed)
        y2, none = ops.t5_ffn_fwd(x, wi, wo, 0.1, seed, need_h=False)
        assert none is None and same_bits(y, y2)
        full = ops.t5_ffn_bwd(x, wi, wo, h, d_y, 0.1, seed)
        for need in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (0, 0, 0)):
            got = ops.t5_ffn_bwd(x, wi, wo, h, d_y, 0.1, seed, need_x=bool(need[0]), need_wi=bool(need[1]),
                                 need_wo=bool(need[2]))
            for n, a, b in zip(need, got, full):
                assert (a is None and not n) or (n and same_bits(a, b)), need


def test_function_matches_the_direct_calls():
    from rqhip import ops
    from rqhip.autograd import T5FFNFunction
    R, L, d, F = 5, 13, 64, 96
    x, wi, wo, d_y = _data(R * L, d, F)
    seed = _seed(9)
    for p in (0.0, 0.1):
        with torch.no_grad():
            y, h = ops.t5_ffn_fwd(x, wi, wo, p, seed)
            g = ops.t5_ffn_bwd(x, wi, wo, h, d_y, p, seed)
        xs, wis, wos = (t.clone().requires_grad_() for t in (x.view(R, L, d), wi, wo))
        out = T5FFNFunction.apply(xs, wis, wos, p, seed)
        assert out.shape == (R, L, d) and same_bits(out.view(-1, d), y)
        d_nc = d_y.view(R, L, d).transpose(0, 1).contiguous().transpose(0, 1)       # non-contiguous upstream gradient
        assert not d_nc.is_contiguous()
        out.backward(d_nc)
        assert same_bits(xs.grad.view(-1, d), g[0]) and same_bits(wis.grad, g[1]) and same_bits(wos.grad, g[2])
        # only the input needs a gradient: frozen weights
        xs = x.clone().requires_grad_()
        T5FFNFunction.apply(xs, wi, wo, p, seed).backward(d_y)
        assert same_bits(xs.grad, g[0])
        # only the weights do
        wis, wos = wi.clone().requires_grad_(), wo.clone().requires_grad_()
        T5FFNFunction.apply(x, wis, wos, p, seed).backward(d_y)
        assert same_bits(wis.grad, g[1]) and same_bits(wos.grad, g[2])


def test_views_off_a_16_byte_boundary_are_realigned():
    """Dense tensors that start one float into a buffer: the kernels' float4 accesses cannot take them, the wrappers copy."""
    from rqhip import ops
    N, d, F = 17, 64, 96
    x, wi, wo, d_y = _data(N, d, F)
    seed = _seed(11)

    def off(t):
        buf = torch.empty(t.numel() + 1, device=t.device)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v

    with torch.no_grad():
        want = ops.t5_ffn_fwd(x, wi, wo, 0.1, seed)
        got = ops.t5_ffn_fwd(off(x), off(wi), off(wo), 0.1, seed)
        assert all(same_bits(a, b) for a, b in zip(want, got))
        want_g = ops.t5_ffn_bwd(x, wi, wo, want[1], d_y, 0.1, seed)
        got_g = ops.t5_ffn_bwd(off(x), off(wi), off(wo), off(want[1]), off(d_y), 0.1, seed)
        assert all(same_bits(a, b) for a, b in zip(want_g, got_g))
        # a transposed weight (not contiguous) is copied too
        got = ops.t5_ffn_fwd(x, wi.t().contiguous().t(), wo, 0.1, seed)
        assert all(same_bits(a, b) for a, b in zip(want, got))


def test_wrappers_reject_what_the_kernel_does_not_take():
    from rqhip import ops
    from rqhip._lib import RqHipError
    dev = torch.device("cuda")
    x, wi, wo = torch.zeros(3, 32, device=dev), torch.zeros(64, 32, device=dev), torch.zeros(32, 64, device=dev)
    with pytest.raises(RqHipError, match="float32"):
        ops.t5_ffn_fwd(x.half(), wi.half(), wo.half())
    with pytest.raises(RqHipError, match="wi must be"):
        ops.t5_ffn_fwd(x, wo, wi)
    with pytest.raises(RqHipError, match="wo must be"):
        ops.t5_ffn_fwd(x, wi, wi)
    with pytest.raises(RqHipError, match="seed"):
        ops.t5_ffn_fwd(x, wi, wo, 0.1)
    with pytest.raises(RqHipError, match="0 <= p < 1"):
        ops.t5_ffn_fwd(x, wi, wo, 1.0, _seed(1))
    with pytest.raises(RqHipError, match="not supported"):
        ops.t5_ffn_fwd(torch.zeros(3, 48, device=dev), torch.zeros(64, 48, device=dev), torch.zeros(48, 64, device=dev))
    with pytest.raises(RqHipError, match="does not match"):
        ops.t5_ffn_bwd(x, wi, wo, torch.zeros(3, 32, device=dev), x)
    with pytest.raises(RqHipError, match="does not match"):
        ops.t5_ffn_bwd(x, wi, wo, torch.zeros(3, 64, device=dev), torch.zeros(2, 32, device=dev))
    # no rows: nothing is launched, the weight gradients are empty sums
    e = torch.zeros(0, 32, device=dev)
    y, h = ops.t5_ffn_fwd(e, wi, wo)
    assert y.shape == (0, 32) and h.shape == (0, 64)
    d_x, d_wi, d_wo = ops.t5_ffn_bwd(e, wi, wo, h, e)
    assert d_x.shape == (0, 32) and d_wi.shape == (64, 32) and d_wo.shape == (32, 64)
    assert not bool(d_wi.any()) and not bool(d_wo.any())
    y, _ = ops.t5_ffn_fwd(torch.zeros(2, 0, 32, device=dev), wi, wo)
    assert y.shape == (2, 0, 32)
