"""ops.rows_pack / ops.rows_unpack (csrc/rows_pack.hip): padded [B, T, d] rows to packed [N, d] rows and back.

Both are copies, so every check is on bits: pack takes the first cu[b + 1] - cu[b] tokens of each row, unpack puts them
back and zero-fills the tails, each is the other's backward (rqhip/autograd.py), and two runs agree.  d covers one 16-byte
piece per token (4), several (32) and the model's width (384); the lengths cover a full row, one token, a middle length
and an empty row."""
import pytest
import torch

from retrieval_cases import same_bits

pytestmark = pytest.mark.gpu

B, T = 3, 5
LENGTHS = {"full, one, three": [5, 1, 3], "with an empty row": [2, 0, 5], "empty first and last": [0, 4, 0]}


def _case(lengths, d, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, d, generator=g)
    x[0, 0, 0] = -0.0                                   # a sign bit a sum with zero would lose
    cu = torch.zeros(B + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(torch.tensor(lengths), 0)
    want = torch.cat([x[b, :n] for b, n in enumerate(lengths)])
    return x.cuda(), cu.cuda(), want.cuda(), int(cu[-1])


@pytest.mark.parametrize("d", [4, 32, 384])
@pytest.mark.parametrize("name", list(LENGTHS))
def test_pack_and_unpack_are_exact_copies(name, d):
    from rqhip import ops
    lengths = LENGTHS[name]
    x, cu, want, N = _case(lengths, d)
    assert ops.rows_pack_supported(torch.float32, d)
    packed = ops.rows_pack(x, cu, N)
    assert packed.shape == (N, d) and same_bits(packed, want)
    back = ops.rows_unpack(packed, cu, B, T)
    assert back.shape == (B, T, d)
    for b, n in enumerate(lengths):
        assert same_bits(back[b, :n], x[b, :n])
        assert same_bits(back[b, n:], torch.zeros(T - n, d, device="cuda"))      # +0.0, every bit
    assert same_bits(ops.rows_pack(x, cu, N), packed) and same_bits(ops.rows_unpack(packed, cu, B, T), back)


@pytest.mark.parametrize("d", [4, 384])
@pytest.mark.parametrize("name", list(LENGTHS))
def test_each_is_the_other_s_backward(name, d):
    from rqhip import ops
    from rqhip.autograd import RowsPackFunction, RowsUnpackFunction
    x, cu, want, N = _case(LENGTHS[name], d)
    g = torch.Generator().manual_seed(1)
    d_packed = torch.randn(N, d, generator=g).cuda()
    d_padded = torch.randn(B, T, d, generator=g).cuda()

    xr = x.clone().requires_grad_()
    packed = RowsPackFunction.apply(xr, cu, N)
    assert same_bits(packed.detach(), want)
    packed.backward(d_packed)
    assert same_bits(xr.grad, ops.rows_unpack(d_packed, cu, B, T))

    pr = want.clone().requires_grad_()
    padded = RowsUnpackFunction.apply(pr, cu, B, T)
    assert same_bits(padded.detach(), ops.rows_unpack(want, cu, B, T))
    padded.backward(d_padded)
    assert same_bits(pr.grad, ops.rows_pack(d_padded, cu, N))


def test_host_checks():
    from rqhip import ops
    from rqhip._lib import RqHipError
    x, cu, want, N = _case(LENGTHS["full, one, three"], 8)
    assert not ops.rows_pack_supported(torch.float32, 6) and not ops.rows_pack_supported(torch.float16, 8)
    with pytest.raises(RqHipError):
        ops.rows_pack(x, cu.long(), N)                      # the table's dtype
    with pytest.raises(RqHipError):
        ops.rows_pack(x, cu[:-1], N)                        # the table's length
    with pytest.raises(RqHipError):
        ops.rows_pack(x, cu, B * T + 1)                     # more packed rows than padded positions
    with pytest.raises(RqHipError):
        ops.rows_unpack(want, cu, B + 1, T)
    with pytest.raises(RqHipError):
        ops.rows_pack(x[..., :6].contiguous(), cu, N)       # d not a multiple of 4
    with pytest.raises(RqHipError):
        ops.rows_pack(x.cpu(), cu, N)
