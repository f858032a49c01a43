"""The trainable fused T5 attention on the host (csrc/t5_attention.hip: rqhip_t5_attention_fwd_train, rqhip_t5_attention_bwd;
ops.t5_attention_dropout_keep; attention_impl = "hip_train"): the argument checks of the C entry points, which all come
before any HIP call, the backward's support table, the dropout hash restated in torch, and the switch's fall-back to the
operators on host tensors.  No GPU needed."""
import math

import pytest
import torch

from retrieval_cases import loss_and_grads, tiny_batch, tiny_model


def _fwd(l, *, R=4, Rk=4, H=6, d_kv=64, Tq=8, Tk=8, ld=None, bias=None, n_delta=0, offset=0, causal=0, p=0.0):
    ld = H * 64 if ld is None else ld
    # every data pointer stays null: they are checked last, so a call that passes every other check launches nothing
    return l.rqhip_t5_attention_fwd_train(None, ld, None, None, ld, R, Rk, H, d_kv, Tq, Tk, bias, n_delta, offset, None,
                                          causal, p, None, None, ld, None, None)


def _bwd(l, *, R=4, Rk=4, H=6, d_kv=64, Tq=8, Tk=8, ld=None, ld_do=None, bias=None, n_delta=0, offset=0, causal=0, p=0.0):
    ld = H * 64 if ld is None else ld
    ld_do = ld if ld_do is None else ld_do
    return l.rqhip_t5_attention_bwd(None, ld, None, None, ld, None, ld, None, None, ld_do, R, Rk, H, d_kv, Tq, Tk, bias,
                                    n_delta, offset, None, causal, p, None, None, None, None, None, None, None)


@pytest.mark.parametrize("call,name", [(_fwd, b"t5_attention_fwd_train"), (_bwd, b"t5_attention_bwd")])
def test_training_pair_argument_checks_without_gpu(call, name):
    from rqhip import _lib
    l = _lib.lib()
    assert call(l, d_kv=32) == -2 and b"d_kv" in l.rqhip_last_error() and name in l.rqhip_last_error()
    assert call(l, d_kv=128) == -2
    assert call(l, Tk=257) == -2 and b"<= 256" in l.rqhip_last_error()
    assert call(l, Tq=257, Tk=256) == -2
    assert call(l, H=0) == -1 and b"bad sizes" in l.rqhip_last_error()
    assert call(l, Tq=0) == -1 and call(l, Tk=0) == -1 and call(l, R=-1, Rk=-1) == -1
    # one K/V per query row: the beams of a beam search are not differentiated
    assert call(l, R=8, Rk=4) == -2 and b"Rk = R" in l.rqhip_last_error()
    assert call(l, R=10, Rk=4) == -2
    assert call(l, ld=6 * 64 - 4) == -1 and b"row strides" in l.rqhip_last_error()
    assert call(l, ld=6 * 64 + 2) == -1
    assert call(l, p=1.0) == -1 and b"0 <= p < 1" in l.rqhip_last_error()
    assert call(l, p=-0.1) == -1 and call(l, p=float("nan")) == -1
    # the bias table must cover every delta j - i of the call
    assert call(l, bias=16, n_delta=14, offset=7) == -1 and b"bias table" in l.rqhip_last_error()
    assert call(l, bias=16, n_delta=15, offset=6) == -1
    assert call(l, Tq=8, Tk=4, causal=1) == -1 and b"exceeds Tk" in l.rqhip_last_error()
    # fully valid sizes, null data: refused last, and by name
    assert call(l) == -1 and b"null pointer" in l.rqhip_last_error()
    assert call(l, bias=16, n_delta=15, offset=7, p=0.1) == -1 and b"null pointer" in l.rqhip_last_error()
    assert call(l, ld=6 * 64 + 4) == -1 and b"null pointer" in l.rqhip_last_error()
    assert call(l, R=0, Rk=0) == 0                       # nothing to do


def test_backward_checks_the_stride_of_d_out():
    from rqhip import _lib
    l = _lib.lib()
    assert _bwd(l, ld_do=6 * 64 - 4) == -1 and b"row strides" in l.rqhip_last_error()
    assert _bwd(l, ld_do=6 * 64 + 1) == -1


def test_backward_supported_truth_table():
    from rqhip import _lib, ops
    l = _lib.lib()
    for H in (1, 6, 8):
        for Tq in (1, 4, 81, 128):
            for Tk in (1, 4, 81, 128):
                assert l.rqhip_t5_attention_bwd_supported(64, H, Tq, Tk) == 1
                assert ops.t5_attention_bwd_supported(torch.float32, 64, H, Tq, Tk)
    assert ops.t5_attention_bwd_supported(torch.float32, 64, 6, 256, 256)     # the stated limit (include/rqhip.h)
    assert not ops.t5_attention_bwd_supported(torch.float32, 64, 6, 257, 16)
    assert not ops.t5_attention_bwd_supported(torch.float32, 64, 6, 16, 257)
    assert not ops.t5_attention_bwd_supported(torch.float32, 32, 6, 16, 16)
    assert not ops.t5_attention_bwd_supported(torch.float32, 128, 6, 16, 16)
    assert not ops.t5_attention_bwd_supported(torch.float32, 64, 0, 16, 16)
    assert not ops.t5_attention_bwd_supported(torch.float32, 64, 6, 0, 16)
    assert not ops.t5_attention_bwd_supported(torch.float32, 64, 6, 16, 0)
    assert not ops.t5_attention_bwd_supported(torch.float16, 64, 6, 16, 16)
    assert not ops.t5_attention_bwd_supported(torch.bfloat16, 64, 6, 16, 16)
    assert not ops.t5_attention_bwd_supported(torch.float64, 64, 6, 16, 16)


def test_dropout_keep_is_a_function_of_seed_and_index():
    from rqhip import ops
    a = ops.t5_attention_dropout_keep(1234, 2, 3, 5, 7, 0.5)
    assert a.dtype == torch.bool and a.shape == (2, 3, 5, 7)
    assert torch.equal(a, ops.t5_attention_dropout_keep(torch.tensor([1234]), 2, 3, 5, 7, 0.5))
    assert not torch.equal(a, ops.t5_attention_dropout_keep(1235, 2, 3, 5, 7, 0.5))
    assert not torch.equal(a, ops.t5_attention_dropout_keep(1234 + (1 << 32), 2, 3, 5, 7, 0.5))   # the seed's high word
    assert bool(ops.t5_attention_dropout_keep(-7, 2, 3, 5, 7, 0.0).all())
    # the decision belongs to the linear index: another factorisation of the same count gives the same bits
    assert torch.equal(a.flatten(), ops.t5_attention_dropout_keep(1234, 1, 6, 7, 5, 0.5).flatten())
    from rqhip._lib import RqHipError
    with pytest.raises(RqHipError):
        ops.t5_attention_dropout_keep(1, 1, 1, 1, 1, 1.0)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_keep_fraction(p):
    from rqhip import ops
    n = 1 << 20
    keep = ops.t5_attention_dropout_keep(99, 8, 8, 128, 128, p)
    assert keep.numel() == n
    kept = int(keep.sum())
    sd = math.sqrt(n * p * (1 - p))
    print(f"p={p}: kept {kept} of {n}, expected {n * (1 - p):.0f}, {abs(kept - n * (1 - p)) / sd:.2f} standard deviations")
    assert abs(kept - n * (1 - p)) <= 5 * sd


def test_dropout_keep_uses_the_low_index_bits():
    from rqhip import ops
    for p in (0.1, 0.5):
        frac = ops.t5_attention_dropout_keep(5, 4, 2, 8, 256, p).float().mean(dim=-1)
        assert bool(((frac > 0) & (frac < 1)).all())


@pytest.mark.parametrize("train", [False, True])
def test_hip_train_on_host_tensors_is_the_operators(train):
    from modules.t5 import ATTENTION_IMPLS
    assert ATTENTION_IMPLS == ("torch", "hip", "hip_train")
    m = tiny_model()
    m.train(train)
    batch = tiny_batch()
    want, want_g = loss_and_grads(m, batch, 3)
    m.attention_impl = "hip_train"
    got, got_g = loss_and_grads(m, batch, 3)
    assert m.encoder.encoder.attention_impl == "hip_train" and m.t5_decoder.attention_impl == "hip_train"
    assert torch.equal(got, want) and sorted(got_g) == sorted(want_g) and len(got_g) > 10
    for n in want_g:
        assert torch.equal(got_g[n], want_g[n]), n
    with torch.no_grad():
        torch.manual_seed(3)
        assert torch.equal(m(batch).loss, want)
    m.attention_impl = "triton"
    with pytest.raises(ValueError, match="attention_impl"):
        m(batch)


def test_hip_train_refuses_a_decode_cache_under_grad():
    from modules.t5 import T5Config, T5Stack
    stack = T5Stack(T5Config(16, d_model=8, num_heads=2, d_ff=8, num_layers=1)).eval()
    stack.attention_impl = "hip_train"
    x = torch.randn(2, 1, 8)
    with pytest.raises(ValueError, match="decode_cache"):
        stack(x, decode_cache=stack.new_decode_cache(3, 2, "cpu"))

    class OnDevice:                # hip_train_active reads only these
        is_cuda, dtype, shape = True, torch.float32, (2, 7, 8)

    assert stack.hip_train_active(OnDevice, 7, None)
    assert not stack.hip_train_active(OnDevice, 300, None)               # beyond the backward's limit
    assert not stack.hip_train_active(torch.zeros(2, 7, 8), 7, None)     # host tensor
    with torch.no_grad():
        assert not stack.hip_train_active(OnDevice, 7, None)             # no_grad: the "hip" rules decide
        assert stack.hip_attention_active(OnDevice, 7, 7)
