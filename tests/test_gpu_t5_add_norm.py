"""The fused residual + dropout + RMS norm on the GPU: ops.t5_add_norm_fwd / ops.t5_add_norm_bwd (csrc/t5_add_norm.hip)
against the operators of modules/t5.py (dropout, residual add, T5LayerNorm, dropout) with the kernel's masks inserted.

x_new is one rounded multiply and one rounded add: bit-exact against the same two torch operators.  n, rstd and the
gradients are gated by retrieval_cases.gate: e = max|a - a64| / max|a64| per tensor, for the kernel and for the
operator chain in fp32 on the same inputs, both against the chain in fp64 (under autograd for the gradients);
e_kernel <= max(4 e_torch, 2^-22) for n and rstd, e_kernel <= max(8 e_torch, 2^-22) for d_x, d_y and d_w.  The floor is
two fp32 ulps of the largest element, for the cases in which the operators happen to be exact.  A tensor whose fp64
reference is exactly zero must be exactly zero.  Measured ratios: profiles/t5_add_norm_error.txt.

Shapes: d = 4 (one lane), 64, 128, 260 (a ragged last float4 group across the lanes), 384 (the model's), 1024 (the
limit); N = 1, 3 / 4 / 5 (the forward's four rows per workgroup), 63 / 64 / 65 (the backward's 64) and 200 (four partial
blocks of the weight gradient, the last one of 8 rows; the partition itself is pinned in test_t5_add_norm_host.py).
Rows: normal, one scaled by 1e-3, one by 1e3, one all zero.  With those rows in a case the 1e3 row sets max|a64| of n,
the all-zero row (rstd = 1000) that of rstd, and the 1e-3 row (rstd about 700) that of d_x and d_y, so
test_ordinary_rows_alone repeats the gates on normal rows only, where every row weighs about the same."""
import pytest
import torch

from retrieval_cases import gate, same_bits, seed as _seed

pytestmark = pytest.mark.gpu

DS = (4, 64, 128, 260, 384, 1024)
NS = (1, 3, 4, 5, 63, 64, 65, 200)
PS = ((0.0, 0.0), (0.1, 0.0), (0.0, 0.1), (0.5, 0.5))
EPS = 1e-6


def _data(N, d, has_x=True, ordinary=False):
    g = torch.Generator().manual_seed(1000 * d + N)
    x, y = torch.randn(N, d, generator=g), torch.randn(N, d, generator=g)
    if N >= 3 and not ordinary:
        x[1] *= 1e-3
        y[1] *= 1e-3
        x[2] *= 1e3
        y[2] *= 1e3
    if N >= 4 and not ordinary:
        x[3] = 0
        y[3] = 0
    w = 1 + 0.5 * torch.randn(d, generator=g)
    w[1::3] = -w[1::3].abs()
    up = torch.randn(2, N, d, generator=g)
    dev = torch.device("cuda")
    return (x.to(dev) if has_x else None), y.to(dev), w.to(dev), up[0].to(dev), up[1].to(dev)


def _masks(seed, N, d, p_in, p_out):
    from rqhip import ops
    keep_in = ops.t5_attention_dropout_keep(seed, 2, 1, N, d, p_in)[0, 0] if p_in > 0 else None
    keep_out = ops.t5_attention_dropout_keep(seed, 2, 1, N, d, p_out)[1, 0] if p_out > 0 else None
    return keep_in, keep_out


def _chain(x, y, w, keep_in, keep_out, p_in, p_out, dtype, d_xnew=None, d_n=None):
    """The operators in `dtype` -> (x_new, n, rstd) and, with an upstream gradient, (d_x or None, d_y, d_w)."""
    y = y.detach().to(dtype).requires_grad_()
    w = w.detach().to(dtype).requires_grad_()
    x = None if x is None else x.detach().to(dtype).requires_grad_()
    t = y if keep_in is None else torch.where(keep_in, y * (1.0 / (1.0 - p_in)), torch.zeros_like(y))
    x_new = t if x is None else x + t
    rstd = torch.rsqrt(x_new.pow(2).mean(-1, keepdim=True) + EPS)          # T5LayerNorm.forward
    n = w * (x_new * rstd)
    if keep_out is not None:
        n = torch.where(keep_out, n * (1.0 / (1.0 - p_out)), torch.zeros_like(n))
    grads = None
    if d_xnew is not None or d_n is not None:
        outs = [o for o, g in ((x_new, d_xnew), (n, d_n)) if g is not None]
        ups = [g.to(dtype) for g in (d_xnew, d_n) if g is not None]
        leaves = ([] if x is None else [x]) + [y, w]
        got = torch.autograd.grad(outs, leaves, ups, allow_unused=True)
        got = [torch.zeros_like(l) if g is None else g for g, l in zip(got, leaves)]
        grads = ([None] if x is None else []) + got
    return x_new.detach(), n.detach(), rstd.detach().squeeze(-1), grads


@pytest.mark.parametrize("has_x", [True, False])
@pytest.mark.parametrize("d", DS)
def test_forward(d, has_x):
    from rqhip import ops
    for N in NS:
        x, y, w, _, _ = _data(N, d, has_x)
        seed = _seed(17 * N + d)
        with torch.no_grad():
            plain = ops.t5_add_norm_fwd(x, y, w, EPS)
        for p_in, p_out in PS:
            name = f"fwd d={d} N={N} x={int(has_x)} p=({p_in}, {p_out})"
            keep_in, keep_out = _masks(seed, N, d, p_in, p_out)
            with torch.no_grad():
                x_new, n, rstd = ops.t5_add_norm_fwd(x, y, w, EPS, p_in, p_out, seed)
                # x_new: one rounded multiply, one rounded add
                t = y if keep_in is None else torch.where(keep_in, y * (1.0 / (1.0 - p_in)), torch.zeros_like(y))
                assert same_bits(x_new, t if x is None else x + t), name
                assert x_new.shape == y.shape and n.shape == y.shape and rstd.shape == (N,)
                if p_out > 0:   # exactly +0 where dropped, elsewhere the undropped n of the same x_new times s_out
                    base = ops.t5_add_norm_fwd(x, y, w, EPS, p_in, 0.0, seed)
                    assert same_bits(base[0], x_new) and same_bits(base[2], rstd), name
                    assert same_bits(n, torch.where(keep_out, base[1] * (1.0 / (1.0 - p_out)), torch.zeros_like(n))), name
                    assert not bool(n.view(torch.int32)[~keep_out].any()), name
                if p_in == 0 and p_out == 0:
                    assert all(same_bits(a, b) for a, b in zip(plain, (x_new, n, rstd))), name
            ref64 = _chain(x, y, w, keep_in, keep_out, p_in, p_out, torch.float64)
            ref32 = _chain(x, y, w, keep_in, keep_out, p_in, p_out, torch.float32)
            gate(f"{name} n", n, ref32[1], ref64[1], 4)
            gate(f"{name} rstd", rstd, ref32[2], ref64[2], 4)
            if N >= 4:           # the all-zero row: rstd = 1 / sqrt(eps), n = 0
                assert not bool(x_new[3].any()) and not bool(n[3].any()), name
                assert abs(float(rstd[3]) - 1000.0) <= 1e-3, name


@pytest.mark.parametrize("d", DS)
def test_backward(d):
    from rqhip import ops
    for N in (1, 5, 63, 64, 65, 200):
        for p_in, p_out in PS:
            for what in ("both", "d_n", "d_xnew", "no x"):
                name = f"bwd d={d} N={N} p=({p_in}, {p_out}) {what}"
                x, y, w, d_xnew, d_n = _data(N, d, what != "no x")
                if what == "d_n":
                    d_xnew = None
                if what == "d_xnew":
                    d_n = None
                seed = _seed(5 * N + d)
                keep_in, keep_out = _masks(seed, N, d, p_in, p_out)
                with torch.no_grad():
                    x_new, n, rstd = ops.t5_add_norm_fwd(x, y, w, EPS, p_in, p_out, seed)
                    d_x, d_y, d_w = ops.t5_add_norm_bwd(x_new, rstd, w, d_n, d_xnew, p_in, p_out, seed,
                                                        need_x=x is not None)
                    both = ops.t5_add_norm_bwd(x_new, rstd, w, d_n, d_xnew, p_in, p_out, seed)
                assert (d_x is None) == (x is None)
                if p_in == 0:
                    assert both[0] is both[1], name
                    assert same_bits(both[0], d_y), name
                else:
                    assert same_bits(both[1], torch.where(keep_in, both[0] * (1.0 / (1.0 - p_in)), torch.zeros_like(d_y))), name
                    assert same_bits(both[1], d_y), name
                assert same_bits(both[2], d_w) and (d_x is None or same_bits(both[0], d_x)), name
                ref64 = _chain(x, y, w, keep_in, keep_out, p_in, p_out, torch.float64, d_xnew, d_n)[3]
                ref32 = _chain(x, y, w, keep_in, keep_out, p_in, p_out, torch.float32, d_xnew, d_n)[3]
                for nm, a, a32, a64 in zip(("d_x", "d_y", "d_w"), (d_x, d_y, d_w), ref32, ref64):
                    if a is not None:
                        gate(f"{name} {nm}", a, a32, a64, 8)


@pytest.mark.parametrize("d", DS)
def test_ordinary_rows_alone(d):
    """The same gates with no scaled and no all-zero row: rstd is about 0.7 in every row, so no single row hides the
    others behind max|a64|."""
    from rqhip import ops
    for N in (5, 65, 200):
        for has_x in (True, False):
            for p_in, p_out in PS:
                name = f"ordinary d={d} N={N} x={int(has_x)} p=({p_in}, {p_out})"
                x, y, w, d_xnew, d_n = _data(N, d, has_x, ordinary=True)
                seed = _seed(7 * N + d)
                keep_in, keep_out = _masks(seed, N, d, p_in, p_out)
                with torch.no_grad():
                    x_new, n, rstd = ops.t5_add_norm_fwd(x, y, w, EPS, p_in, p_out, seed)
                    grads = ops.t5_add_norm_bwd(x_new, rstd, w, d_n, d_xnew, p_in, p_out, seed, need_x=has_x)
                ref64 = _chain(x, y, w, keep_in, keep_out, p_in, p_out, torch.float64, d_xnew, d_n)
                ref32 = _chain(x, y, w, keep_in, keep_out, p_in, p_out, torch.float32, d_xnew, d_n)
                assert same_bits(x_new, ref32[0]), name
                gate(f"{name} n", n, ref32[1], ref64[1], 4)
                gate(f"{name} rstd", rstd, ref32[2], ref64[2], 4)
                for nm, a, a32, a64 in zip(("d_x", "d_y", "d_w"), grads, ref32[3], ref64[3]):
                    if a is not None:
                        gate(f"{name} {nm}", a, a32, a64, 8)


@pytest.mark.parametrize("d", DS)
def test_same_bits_twice_and_rows_do_not_depend_on_the_batch(d):
    from rqhip import ops
    N = NS[-1]
    x, y, w, d_xnew, d_n = _data(N, d)

    def run(p_in, p_out, seed, rows=slice(None)):
        xr, yr, un, ux = x[rows], y[rows], d_n[rows], d_xnew[rows]
        with torch.no_grad():
            x_new, n, rstd = ops.t5_add_norm_fwd(xr, yr, w, EPS, p_in, p_out, seed)
            return (x_new, n, rstd) + tuple(ops.t5_add_norm_bwd(x_new, rstd, w, un, ux, p_in, p_out, seed))

    for p_in, p_out in PS:
        a, b = run(p_in, p_out, _seed(3)), run(p_in, p_out, _seed(3))
        assert all(same_bits(u, v) for u, v in zip(a, b)), (p_in, p_out)
    whole = run(0.0, 0.0, None)
    for r in (0, 1, 2, 3, 62, 63, 64, 67, 199):
        one = run(0.0, 0.0, None, slice(r, r + 1))
        for k in (0, 1, 2, 3):       # x_new, n, rstd, d_x
            assert same_bits(whole[k][r:r + 1], one[k]), (r, k)
    # another seed, other masks: x_new carries keep_in, n keep_out
    a, b = run(0.5, 0.0, _seed(3)), run(0.5, 0.0, _seed(4))
    assert not same_bits(a[0], b[0])
    a, b = run(0.0, 0.5, _seed(3)), run(0.0, 0.5, _seed(4))
    assert same_bits(a[0], b[0]) and not same_bits(a[1], b[1])
    keep = ops.t5_attention_dropout_keep(_seed(3), 2, 1, N, d, 0.5)
    assert not torch.equal(keep[0], keep[1])          # the two planes of one seed differ too


def test_function_matches_the_direct_calls():
    from rqhip import ops
    from rqhip.autograd import T5AddNormFunction
    N, d = 65, 384
    x, y, w, d_xnew, d_n = _data(N, d)
    seed = _seed(9)
    for p_in in (0.0, 0.1):
        xs, ys, ws = (t.clone().requires_grad_() for t in (x, y, w))
        x_new, n = T5AddNormFunction.apply(xs, ys, ws, EPS, p_in, 0.1, seed)
        torch.autograd.backward([x_new, n], [d_xnew, d_n])
        with torch.no_grad():
            f = ops.t5_add_norm_fwd(x, y, w, EPS, p_in, 0.1, seed)
            g = ops.t5_add_norm_bwd(f[0], f[2], w, d_n, d_xnew, p_in, 0.1, seed)
        assert same_bits(x_new, f[0]) and same_bits(n, f[1])
        assert same_bits(xs.grad, g[0]) and same_bits(ys.grad, g[1]) and same_bits(ws.grad, g[2])
        # only n used, x absent, a non-contiguous upstream gradient
        ys.grad = ws.grad = None
        _, n = T5AddNormFunction.apply(None, ys, ws, EPS, p_in, 0.1, seed)
        d_nc = d_n.t().contiguous().t()
        assert not d_nc.is_contiguous()
        n.backward(d_nc)
        with torch.no_grad():
            f = ops.t5_add_norm_fwd(None, y, w, EPS, p_in, 0.1, seed)
            g = ops.t5_add_norm_bwd(f[0], f[2], w, d_n, None, p_in, 0.1, seed, need_x=False)
        assert g[0] is None and same_bits(ys.grad, g[1]) and same_bits(ws.grad, g[2])


def test_views_off_a_16_byte_boundary_are_realigned():
    """Dense rows that start one float into a buffer: the kernels' float4 accesses cannot take them, the wrappers copy."""
    from rqhip import ops
    N, d = 5, 64
    x, y, w, d_xnew, d_n = _data(N, d)
    seed = _seed(11)

    def off(t):
        buf = torch.empty(t.numel() + 1, device=t.device)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v

    with torch.no_grad():
        want = ops.t5_add_norm_fwd(x, y, w, EPS, 0.1, 0.1, seed)
        got = ops.t5_add_norm_fwd(off(x), off(y), off(w), EPS, 0.1, 0.1, seed)
        assert all(same_bits(a, b) for a, b in zip(want, got))
        want_g = ops.t5_add_norm_bwd(want[0], want[2], w, d_n, d_xnew, 0.1, 0.1, seed)
        got_g = ops.t5_add_norm_bwd(off(want[0]), off(want[2]), off(w), off(d_n), off(d_xnew), 0.1, 0.1, seed)
        assert all(same_bits(a, b) for a, b in zip(want_g, got_g))


def test_wrappers_reject_what_the_kernel_does_not_take():
    from rqhip import ops
    from rqhip._lib import RqHipError
    dev = torch.device("cuda")
    y, w = torch.zeros(3, 8, device=dev), torch.ones(8, device=dev)
    with pytest.raises(RqHipError, match="float32"):
        ops.t5_add_norm_fwd(None, y.half(), w.half(), EPS)
    with pytest.raises(RqHipError, match="does not match"):
        ops.t5_add_norm_fwd(torch.zeros(2, 8, device=dev), y, w, EPS)
    with pytest.raises(RqHipError, match="seed"):
        ops.t5_add_norm_fwd(None, y, w, EPS, 0.1, 0.0)
    with pytest.raises(RqHipError, match="multiples of 4"):
        ops.t5_add_norm_fwd(None, torch.zeros(3, 6, device=dev), torch.ones(6, device=dev), EPS)
    with pytest.raises(RqHipError, match="w must be"):
        ops.t5_add_norm_fwd(None, y, torch.ones(4, device=dev), EPS)
    out = ops.t5_add_norm_fwd(None, torch.zeros(0, 8, device=dev), w, EPS)
    assert out[0].shape == (0, 8) and out[2].shape == (0,)
