"""The dropout scale 1 / (1 - p) of the T5 kernels, bit for bit (csrc/t5_common.h: dropout_scale_f32, dropout_scale_f64).

The scale exists in two roundings.  The attention pair computes it in fp32, 1.0f / (1.0f - (float)p); t5_add_norm and
t5_ffn evaluate 1 / (1 - p) in double and round once (include/rqhip.h).  The two agree at p = 0.1 and 0.5, the only
probabilities the other tests use, and differ at p = 0.15 and p = 0.6, which are used here.

Every shape makes the expected value exact: one product per output element and every other term an exact zero, so a
kept element is `value * s` rounded once and a dropped one is +0, and the comparison is on the bits.  Each test also
asserts that its mask (ops.t5_attention_dropout_keep, seed 1234) keeps some elements and drops some, and that the other
rounding of the scale would have given a different tensor: it cannot pass by accident."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 1234
PS = (0.15, 0.6)


def _scale_f32(p):
    return float(np.float32(1) / (np.float32(1) - np.float32(p)))


def _scale_f64(p):
    return float(np.float32(1.0 / (1.0 - p)))


def _seed():
    return torch.tensor([SEED], dtype=torch.int64, device="cuda")


def _pin(name, got, values, keep, s, s_other):
    """got == (keep ? values * s : +0) in bits; `values` and `keep` on the host, broadcast to got's shape."""
    assert s != s_other
    keep = keep.expand(got.shape)
    assert bool(keep.any()) and not bool(keep.all()), f"{name}: the mask must keep some elements and drop some"
    zero = torch.zeros(got.shape)
    want, other = torch.where(keep, values * s, zero), torch.where(keep, values * s_other, zero)
    differ = int((want != other).sum())
    print(f"{name}: {int(keep.sum())} of {keep.numel()} kept, {differ} products differ under the other rounding")
    assert differ > 0, f"{name}: the two roundings give the same tensor, the test pins nothing"
    assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)), name


def _attention_data(R, H, Tq, Tk):
    g = torch.Generator().manual_seed(7)
    return [torch.randn(R, T, H * 64, generator=g) for T in (Tq, Tk, Tk, Tq)]     # q, k, v, d_out


@pytest.mark.parametrize("p", PS)
def test_attention_forward_scales_in_fp32(p):
    """One key: its weight is exactly 1, so out[r, i, head h] = v[r, 0, head h] * s where keep[r, h, i, 0]."""
    from rqhip import ops
    R, H, Tq = 2, 2, 4
    q, k, v, _ = _attention_data(R, H, Tq, 1)
    out, _ = ops.t5_attention_fwd_train(q.cuda(), k.cuda(), v.cuda(), H, p=p, seed=_seed())
    keep = ops.t5_attention_dropout_keep(SEED, R, H, Tq, 1, p)[..., 0].permute(0, 2, 1)[..., None]     # [R, Tq, H, 1]
    _pin("out", out.view(R, Tq, H, 64), v.view(R, 1, H, 64), keep, _scale_f32(p), _scale_f64(p))


@pytest.mark.parametrize("p", PS)
def test_attention_backward_scales_in_fp32(p):
    """One query and one key: dv = d_out * s where kept; dS = 0 for a row with one live key, so dq = dk = 0."""
    from rqhip import ops
    R, H = 8, 2
    q, k, v, d_out = _attention_data(R, H, 1, 1)
    q, k, v = q.cuda(), k.cuda(), v.cuda()
    out, lse = ops.t5_attention_fwd_train(q, k, v, H, p=p, seed=_seed())
    dq, dk, dv, dtable = ops.t5_attention_bwd(q, k, v, out, lse, d_out.cuda(), H, p=p, seed=_seed())
    keep = ops.t5_attention_dropout_keep(SEED, R, H, 1, 1, p).view(R, 1, H, 1)
    _pin("dv", dv.view(R, 1, H, 64), d_out.view(R, 1, H, 64), keep, _scale_f32(p), _scale_f64(p))
    assert dtable is None and not bool(dq.any()) and not bool(dk.any())


@pytest.mark.parametrize("p", PS)
def test_add_norm_scales_in_double(p):
    """Without a residual x_new = dropout(y, p_in); behind the norm n = dropout(n at p_out = 0, p_out)."""
    from rqhip import ops
    N, d = 4, 8
    g = torch.Generator().manual_seed(8)
    y, w = torch.randn(N, d, generator=g), 1 + 0.5 * torch.randn(d, generator=g)
    keep = ops.t5_attention_dropout_keep(SEED, 2, 1, N, d, p)
    x_new, _, _ = ops.t5_add_norm_fwd(None, y.cuda(), w.cuda(), 1e-6, p, 0.0, _seed())
    _pin("x_new", x_new, y, keep[0, 0], _scale_f64(p), _scale_f32(p))
    _, n0, _ = ops.t5_add_norm_fwd(None, y.cuda(), w.cuda(), 1e-6, 0.0, 0.0)
    _, n, _ = ops.t5_add_norm_fwd(None, y.cuda(), w.cuda(), 1e-6, 0.0, p, _seed())
    _pin("n", n, n0.cpu(), keep[1, 0], _scale_f64(p), _scale_f32(p))


@pytest.mark.parametrize("p", PS)
def test_ffn_scales_in_double(p):
    """Identity weights and positive rows: h = x, and y = dropout(x, p)."""
    from rqhip import ops
    N, d = 4, 32
    x = 0.5 + 1.5 * torch.rand(N, d, generator=torch.Generator().manual_seed(9))
    eye = torch.eye(d, device="cuda")
    y, h = ops.t5_ffn_fwd(x.cuda(), eye, eye, p, _seed())
    assert torch.equal(h.cpu(), x)
    _pin("y", y, x, ops.t5_attention_dropout_keep(SEED, 1, 1, N, d, p)[0, 0], _scale_f64(p), _scale_f32(p))
