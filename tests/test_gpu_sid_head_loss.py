"""The fused semantic-id heads + cross-entropy on the GPU: ops.sid_head_loss_fwd / _bwd and autograd.SidHeadLossFunction
(csrc/sid_head_loss.hip) against torch's own F.linear / F.cross_entropy in fp64.

Gates: retrieval_cases.gate, e = max|a - a64| / max|a64| per tensor, e_kernel <= max(4 e_torch, 2^-22) for
loss_d and max(8 e_torch, 2^-22) for d_x and each d_w[h]; e_torch from the same operators in fp32 on the same device with
the same inputs.  Every gated value is printed: profiles/sid_head_loss_error.txt is that output.  Everything the header
promises about bits (run-to-run, strides, unread positions and columns, independence of the levels, out-of-range
targets, graph replay) is checked without a tolerance."""
import functools

import pytest
import torch
import torch.nn.functional as F

from retrieval_cases import bits, gate

pytestmark = pytest.mark.gpu

# (B, K, d, L, T): the smallest sizes at which row blocks of 8, code blocks of 8, 64-row blocks of d_w, 256 codes or
# columns per pass and their tails can go wrong, and the workload's own (64, 256, 384, 3, 4)
CASES = [(1, 1, 4, 1, 1), (1, 2, 4, 1, 2), (2, 3, 8, 2, 3), (4, 16, 16, 8, 9), (3, 32, 64, 3, 4), (16, 32, 128, 3, 4),
         (17, 100, 260, 3, 6), (63, 64, 32, 3, 4), (64, 256, 384, 3, 4), (65, 256, 128, 4, 5), (65, 257, 64, 3, 4),
         (200, 32, 1024, 3, 4), (5, 1000, 64, 2, 3), (5, 1024, 64, 1, 2)]
SCALED = [((64, 256, 384, 3, 4), 8.0), ((64, 256, 384, 3, 4), 0.05)]
BITS = [(2, 3, 8, 2, 3), (17, 100, 260, 3, 6), (65, 257, 64, 3, 4)]     # the cases of the exact checks


def _same(a, b):
    return (a is None and b is None) or torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def _inputs(case, scale=1.0):
    """x [B, T, d], L weights [K, d] and target [B, L + 1] (the last column is never read) on the host."""
    B, K, d, L, T = case
    g = torch.Generator().manual_seed(B * 1000003 + K * 1009 + d * 31 + L)
    x = torch.randn(B, T, d, generator=g) * scale
    ws = tuple(torch.randn(K, d, generator=g) * (scale / d ** 0.5) for _ in range(L))
    target = torch.randint(0, K, (B, L + 1), generator=g)
    target[0, 0], target[-1, L - 1] = 0, K - 1
    return x, ws, target


def _operators(x, ws, target, L, d_loss=1.0):
    """(loss_d, d_x, d_w) of the model's own operator sequence at the inputs' precision and device."""
    x = x.detach().clone().requires_grad_(True)
    ws = [w.detach().clone().requires_grad_(True) for w in ws]
    total = torch.zeros((), dtype=x.dtype, device=x.device)
    loss_d = []
    for h in range(L):
        h_loss = F.cross_entropy(F.linear(x[:, h], ws[h]), target[:, h])
        total = total + h_loss
        loss_d.append(h_loss.detach())
    total.backward(torch.full_like(total, d_loss))
    return torch.stack(loss_d), x.grad, [w.grad for w in ws]


@functools.lru_cache(maxsize=None)
def _reference(case, scale=1.0, d_loss=1.0):
    x, ws, target = _inputs(case, scale)
    return _operators(x.double(), [w.double() for w in ws], target, case[3], d_loss)


def _fused(x, ws, target, d_loss=None, x_grad=True, frozen=()):
    """(loss, loss_d, d_x, d_w) of one SidHeadLossFunction call and its backward."""
    from rqhip.autograd import SidHeadLossFunction
    x = x.detach().requires_grad_(x_grad)
    ws = [w.detach().requires_grad_(h not in frozen) for h, w in enumerate(ws)]
    loss, loss_d = SidHeadLossFunction.apply(x, target, *ws)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.requires_grad
    assert loss_d.shape == (len(ws),) and not loss_d.requires_grad
    loss.backward(None if d_loss is None else torch.full_like(loss, d_loss))
    return loss.detach(), loss_d, x.grad, [w.grad for w in ws]


def _on_device(case, scale=1.0):
    dev = torch.device("cuda")
    x, ws, target = _inputs(case, scale)
    return x.to(dev), [w.to(dev) for w in ws], target.to(dev)


def _ordered_sum(loss_d):
    total = torch.zeros((), dtype=torch.float32, device=loss_d.device)
    for h in range(loss_d.shape[0]):
        total = total + loss_d[h]
    return total


@pytest.mark.parametrize("case,scale,d_loss", [(c, 1.0, 1.0) for c in CASES] + [(c, s, 1.0) for c, s in SCALED]
                         + [((17, 100, 260, 3, 6), 1.0, 0.5), ((64, 256, 384, 3, 4), 1.0, 0.5)])
def test_against_fp64(case, scale, d_loss):
    B, K, d, L, T = case
    x, ws, target = _on_device(case, scale)
    loss_d64, dx64, dw64 = _reference(case, scale, d_loss)
    loss_d32, dx32, dw32 = _operators(x, ws, target, L, d_loss)
    loss, loss_d, d_x, d_w = _fused(x, ws, target, None if d_loss == 1.0 else d_loss)
    name = f"B{B} K{K} d{d} L{L} T{T} scale {scale:g} d_loss {d_loss:g}"
    if scale == 8.0:
        assert float(F.linear(x[:, 0], ws[0]).abs().max()) > 100      # logits that need the stable softmax
    if scale == 0.05:
        assert abs(float(loss_d64[0]) - 5.545) < 0.01                 # ln 256
    gate(f"{name} loss_d", loss_d, loss_d32, loss_d64, 4)
    gate(f"{name} d_x", d_x, dx32, dx64, 8)
    for h in range(L):
        gate(f"{name} d_w[{h}]", d_w[h], dw32[h], dw64[h], 8)
    # bits: the loss is the levels in torch's order, unread positions get exact zeros, a second run repeats every bit
    assert _same(loss, _ordered_sum(loss_d))
    assert d_x.shape == (B, T, d) and d_x.is_contiguous() and not bool(d_x[:, L:].any())
    again = _fused(x, ws, target, None if d_loss == 1.0 else d_loss)
    assert _same(again[0], loss) and _same(again[1], loss_d) and _same(again[2], d_x)
    assert all(_same(a, b) for a, b in zip(again[3], d_w))


@pytest.mark.parametrize("case", BITS)
def test_unread_positions_and_columns_change_no_bit(case):
    B, K, d, L, T = case
    x, ws, target = _on_device(case)
    want = _fused(x, ws, target)
    x2, t2 = x.clone(), target.clone()
    x2[:, L:] = float("nan")
    t2[:, L:] = K + 5
    got = _fused(x2, ws, t2)
    assert all(_same(a, b) for a, b in zip(got[:3], want[:3])) and all(_same(a, b) for a, b in zip(got[3], want[3]))


@pytest.mark.parametrize("case", BITS)
def test_strided_inputs_give_the_bits_of_their_copies(case, monkeypatch):
    from rqhip import ops
    B, K, d, L, T = case
    x, ws, target = _on_device(case)
    want = _fused(x, ws, target)
    wide = torch.full((B, T + 2, d + 8), float("nan"), device=x.device)
    wide[:, 1:T + 1, 4:d + 4] = x
    xs = wide[:, 1:T + 1, 4:d + 4]
    tw = torch.full((B, 2 * L + 3), -7, dtype=torch.long, device=x.device)
    tw[:, 1:L + 2] = target
    ts = tw[:, 1:L + 2]
    assert not xs.is_contiguous() and not ts.is_contiguous() and xs.data_ptr() % 16 == 0
    seen = []
    handle = ops._lib.lib()
    o_fwd = handle.rqhip_sid_head_loss_fwd

    def fwd(*a):                    # the strides reach the C entry point: nothing was copied on the way
        seen.append((a[0], a[1], a[2], a[4], a[5]))
        return o_fwd(*a)

    monkeypatch.setattr(handle, "rqhip_sid_head_loss_fwd", fwd)
    got = _fused(xs, ws, ts)
    monkeypatch.undo()
    assert seen == [(xs.data_ptr(), (T + 2) * (d + 8), d + 8, ts.data_ptr(), 2 * L + 3)]
    assert all(_same(a, b) for a, b in zip(got[:3], want[:3])) and all(_same(a, b) for a, b in zip(got[3], want[3]))
    # an int32 target is converted
    got = _fused(x, ws, target.int())
    assert all(_same(a, b) for a, b in zip(got[:3], want[:3]))


@pytest.mark.parametrize("case", [(17, 100, 260, 3, 6), (65, 257, 64, 3, 4)])
def test_a_level_depends_on_its_own_targets_only(case):
    B, K, d, L, T = case
    x, ws, target = _on_device(case)
    _, loss_d, d_x, d_w = _fused(x, ws, target)
    t2 = target.clone()
    t2[:, 1] = (t2[:, 1] + 1) % K
    _, loss_d2, d_x2, d_w2 = _fused(x, ws, t2)
    assert not _same(loss_d[1], loss_d2[1]) and not _same(d_w[1], d_w2[1])
    for h in (0, 2):
        assert _same(loss_d[h], loss_d2[h]) and _same(d_x[:, h], d_x2[:, h]) and _same(d_w[h], d_w2[h])


def test_gradient_routing():
    from rqhip import ops
    case = (17, 100, 260, 3, 6)
    x, ws, target = _on_device(case)
    loss, loss_d, d_x, d_w = _fused(x, ws, target)
    got = _fused(x, ws, target, x_grad=False)
    assert got[2] is None and _same(got[0], loss) and all(_same(a, b) for a, b in zip(got[3], d_w))
    got = _fused(x, ws, target, frozen=(1,))
    assert got[3][1] is None and _same(got[2], d_x) and _same(got[3][0], d_w[0]) and _same(got[3][2], d_w[2])
    got = _fused(x, ws, target, x_grad=True, frozen=(0, 1, 2))
    assert got[3] == [None, None, None] and _same(got[2], d_x)
    with torch.no_grad():
        out = ops.sid_head_loss_fwd(x, ws, target, 3)
    assert _same(out[0], loss) and _same(out[1], loss_d) and not out[0].requires_grad


@pytest.mark.parametrize("bad", [-1, 32, -100, 2 ** 40])
def test_out_of_range_target(bad):
    case = (3, 32, 64, 3, 4)
    x, ws, target = _on_device(case)
    loss, loss_d, d_x, d_w = _fused(x, ws, target)
    t2 = target.clone()
    t2[1, 1] = bad
    loss2, loss_d2, d_x2, d_w2 = _fused(x, ws, t2)
    assert bool(torch.isnan(loss_d2[1])) and bool(torch.isnan(loss2))
    for h in (0, 2):
        assert _same(loss_d2[h], loss_d[h]) and _same(d_x2[:, h], d_x[:, h]) and _same(d_w2[h], d_w[h])
    # the row has no one-hot term: its gradient is the softmax's alone, every other row keeps its bits
    assert bool(torch.isfinite(d_x2).all()) and bool(torch.isfinite(d_w2[1]).all())
    assert _same(d_x2[0], d_x[0]) and _same(d_x2[2], d_x[2]) and not bool(d_x2[:, 3:].any())
    assert float(d_x2[1, 1].abs().max()) > 0


def test_graph_capture_replays_new_inputs():
    from rqhip import ops
    case = (17, 100, 260, 3, 6)
    L = case[3]
    x, ws, target = _on_device(case)
    g = torch.Generator().manual_seed(5)
    x_new = torch.randn(x.shape, generator=g).to(x.device)
    t_new = torch.randint(0, case[1], target.shape, generator=g).to(x.device)
    up = torch.full((), 0.25, device=x.device)

    def pair(x, target):
        loss, loss_d, z, lse = ops.sid_head_loss_fwd(x, ws, target, L)
        d_x, d_w = ops.sid_head_loss_bwd(x, ws, target, z, lse, up, L)
        return [loss, loss_d, d_x, *d_w]

    eager = [t.clone() for t in pair(x_new, t_new)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            pair(x, target)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = pair(x, target)
    x.copy_(x_new)
    target.copy_(t_new)
    graph.replay()
    torch.cuda.synchronize()
    assert len(captured) == len(eager) == 3 + L
    assert all(_same(a, b) for a, b in zip(captured, eager))
