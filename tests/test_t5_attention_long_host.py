"""The fused T5 attention beyond 256 tokens (csrc/t5_attention_long.hip, ops.t5_attention_long*, the
`attention_long_impl` switch) on the host: its support table, the argument checks of the C entry points (each returns
before any device call and names its limit in rqhip_last_error), the size of the backward's workspace, and the dispatch
predicates of a stack with the switch on, off and unknown.  No GPU needed."""
import pytest
import torch

from retrieval_cases import tiny_model

OK_PTR = 4096      # a non-null, 16-byte aligned address that is never dereferenced: every check below fails before a launch
ODD_PTR = 4096 + 8


def _fwd(l, *, ptr=OK_PTR, R=4, Rk=4, H=6, d_kv=64, Tq=300, Tk=300, ld=None, past=0, anc=None, bias=None, n_delta=0,
         offset=0, causal=0):
    ld = H * 64 if ld is None else ld
    return l.rqhip_t5_attention_long(ptr, ld, OK_PTR, OK_PTR, ld, R, Rk, H, d_kv, Tq, Tk, bias, n_delta, offset, None,
                                     causal, past, anc, OK_PTR, ld, None)


def _train(l, *, ptr=OK_PTR, R=4, Rk=4, H=6, Tq=300, Tk=300, ld=None, bias=None, n_delta=0, offset=0, causal=0, p=0.0):
    ld = H * 64 if ld is None else ld
    return l.rqhip_t5_attention_long_fwd_train(ptr, ld, OK_PTR, OK_PTR, ld, R, Rk, H, 64, Tq, Tk, bias, n_delta, offset,
                                               None, causal, p, None, OK_PTR, ld, OK_PTR, OK_PTR, None)


def _bwd(l, *, ptr=OK_PTR, R=4, Rk=4, H=6, Tq=300, Tk=300, ld=None, bias=None, n_delta=0, offset=0, causal=0, ws=OK_PTR,
         ws_bytes=None):
    ld = H * 64 if ld is None else ld
    if ws_bytes is None:
        ws_bytes = l.rqhip_t5_attention_long_bwd_workspace_bytes(R, H, Tq, Tk)
    return l.rqhip_t5_attention_long_bwd(ptr, ld, OK_PTR, OK_PTR, ld, OK_PTR, ld, OK_PTR, OK_PTR, OK_PTR, ld, R, Rk, H, 64,
                                         Tq, Tk, bias, n_delta, offset, None, causal, 0.0, None, OK_PTR, OK_PTR, OK_PTR,
                                         OK_PTR if bias else None, ws, ws_bytes, None)


def test_long_supported_truth_table():
    from rqhip import _lib, ops
    l = _lib.lib()
    lengths = (1, 256, 257, 2048)
    for H in (1, 6, 64):
        for Tq in lengths:
            for Tk in lengths:
                assert l.rqhip_t5_attention_long_supported(64, H, Tq, Tk) == 1
                assert ops.t5_attention_long_supported(torch.float32, 64, H, Tq, Tk)
    for Tq, Tk in ((2049, 16), (16, 2049), (0, 16), (16, 0)):
        assert not ops.t5_attention_long_supported(torch.float32, 64, 6, Tq, Tk)
    assert not ops.t5_attention_long_supported(torch.float32, 32, 6, 300, 300)
    assert not ops.t5_attention_long_supported(torch.float32, 128, 6, 300, 300)
    assert not ops.t5_attention_long_supported(torch.float32, 64, 0, 300, 300)
    for dtype in (torch.float16, torch.bfloat16, torch.float64, torch.int32):
        assert not ops.t5_attention_long_supported(dtype, 64, 6, 300, 300)
    assert ops.T5_ATTENTION_LONG_CHUNK == 128 and ops.T5_ATTENTION_LONG_QBLOCK == 64


def test_long_argument_checks_without_gpu():
    from rqhip import _lib
    l = _lib.lib()
    err = l.rqhip_last_error
    # dense K/V at past = 0 only
    assert _fwd(l, past=1) == -2 and b"past = 0" in err()
    assert _fwd(l, anc=OK_PTR) == -2 and b"ancestor" in err()
    # the limits
    assert _fwd(l, Tk=2049) == -2 and b"<= 2048" in err()
    assert _fwd(l, Tq=2049, Tk=2048) == -2 and b"<= 2048" in err()
    assert _train(l, Tk=2049) == -2 and b"<= 2048" in err()
    assert _bwd(l, Tk=2049) == -2 and b"<= 2048" in err()
    assert _fwd(l, d_kv=32) == -2 and b"d_kv = 64" in err()
    assert _fwd(l, H=0) == -1 and _fwd(l, Tq=0) == -1 and _fwd(l, Tk=0) == -1
    assert _fwd(l, R=10, Rk=4) == -1 and b"multiple" in err()
    # pointers: null, then misaligned
    assert _fwd(l, ptr=None) == -1 and b"null pointer" in err()
    assert _train(l, ptr=None) == -1 and b"null pointer" in err()
    assert _bwd(l, ptr=None) == -1 and b"null pointer" in err()
    assert _train(l, p=0.5) == -1 and b"seed" in err()          # dropout without a seed
    for call in (_fwd, _train, _bwd):
        assert call(l, ptr=ODD_PTR) == -1 and b"16-byte aligned" in err()
    assert _bwd(l, ws=ODD_PTR) == -1 and b"16-byte aligned" in err()
    # strides
    for call in (_fwd, _train, _bwd):
        assert call(l, ld=6 * 64 + 2) == -1 and b"multiples of 4" in err()
        assert call(l, ld=6 * 64 - 4) == -1 and b"H * 64" in err()
    # Tq > Tk goes with neither causal nor a bias table
    for call in (_fwd, _train, _bwd):
        assert call(l, Tq=300, Tk=299, causal=1) == -1 and b"exceeds Tk" in err()
        assert call(l, Tq=300, Tk=299, bias=OK_PTR, n_delta=598, offset=299) == -1 and b"exceeds Tk" in err()
    # the bias table must cover every delta of the call
    assert _fwd(l, bias=OK_PTR, n_delta=598, offset=299) == -1 and b"bias table" in err()
    assert _fwd(l, bias=OK_PTR, n_delta=599, offset=298) == -1 and b"bias table" in err()
    # the training pair takes one K/V per row
    assert _train(l, R=4, Rk=2) == -2 and b"Rk = R" in err()
    assert _bwd(l, R=4, Rk=2) == -2 and b"Rk = R" in err()
    # the workspace
    need = l.rqhip_t5_attention_long_bwd_workspace_bytes(4, 6, 300, 300)
    assert _bwd(l, ws_bytes=need - 1) == -1 and b"workspace" in err() and str(need).encode() in err()
    assert _bwd(l, ws=None) == -1 and b"null pointer" in err()
    # nothing to do
    assert _fwd(l, R=0, Rk=0) == 0 and _train(l, R=0, Rk=0) == 0 and _bwd(l, R=0, Rk=0) == 0


def test_long_workspace_grows_with_the_sum_of_the_lengths_not_their_product():
    from rqhip import _lib
    ws = _lib.lib().rqhip_t5_attention_long_bwd_workspace_bytes
    base = ws(2, 3, 512, 512)
    assert base > 0
    assert ws(4, 3, 512, 512) == 2 * base and ws(2, 6, 512, 512) == 2 * base      # linear in R and in H
    assert ws(2, 3, 512, 1024) > base and ws(2, 3, 1024, 512) > base
    # D [R, H, Tq] and at most four [Tq + Tk - 1] rows per (row, head): five floats per token of Tq + Tk bound it
    for T in (257, 512, 1024, 2048):
        assert ws(2, 3, T, T) <= 2 * 3 * 5 * (T + T) * 4
        assert ws(2, 3, 1, T) <= 2 * 3 * 5 * (1 + T) * 4
    assert ws(2, 3, 2048, 2048) <= 4 * base + 1024                                 # 4 x the lengths: 4 x, not 16 x
    assert ws(2, 3, 2048, 2048) < 2 * 3 * 2048 * 2048 * 4 // 50                      # far below one score tensor
    assert ws(0, 3, 512, 512) == 0


class OnDevice:                # the predicates read only these
    is_cuda, dtype = True, torch.float32


def _stack(is_decoder=False):
    from modules.t5 import T5Config, T5Stack
    return T5Stack(T5Config(16, d_model=8, num_heads=2, d_ff=8, num_layers=1, is_decoder=is_decoder)).eval()


def test_long_dispatch_predicates_on_a_stack():
    stack = _stack()
    assert stack.attention_long_impl == "torch"
    stack.attention_impl = "hip"
    with torch.no_grad():
        assert not stack.hip_attention_active(OnDevice, 7, 300)            # the default: today's answers
        assert not stack.hip_attention_active(OnDevice, 1, 3, 300)
        stack.attention_long_impl = "hip"
        assert stack.hip_attention_active(OnDevice, 7, 300)
        assert stack.hip_attention_active(OnDevice, 1, 3, 300)
        assert stack.hip_attention_active(OnDevice, 7, 7)                   # the short lengths as before
        assert not stack.hip_attention_active(OnDevice, 7, 2049)           # beyond the long kernel too
        assert not stack.hip_attention_active(OnDevice, 1, 3, 2049)
        assert not stack.hip_attention_active(OnDevice, 1, 300, 300, cached=True)   # a decode cache is the short kernel's
        assert not stack.hip_attention_active(torch.zeros(1, 7, 8), 7, 300)  # host tensor
        stack.attention_impl = "torch"
        assert not stack.hip_attention_active(OnDevice, 7, 300)            # the long switch alone selects nothing
    stack.attention_impl = "hip_train"
    assert stack.hip_train_active(OnDevice, 300, None)
    assert not stack.hip_train_active(OnDevice, 2049, None)
    stack.attention_long_impl = "torch"
    assert not stack.hip_train_active(OnDevice, 300, None)
    assert stack.hip_train_active(OnDevice, 256, None)


def test_long_dispatch_predicate_of_a_decoder_under_grad():
    stack = _stack(is_decoder=True)
    stack.attention_impl = "hip_train"

    class X(OnDevice):
        shape = (3, 4, 8)

    cross = [(torch.zeros(3, 2, 300, 64), torch.zeros(3, 2, 300, 64))]
    assert not stack.hip_train_active(X, 4, cross)
    stack.attention_long_impl = "hip"
    assert stack.hip_train_active(X, 4, cross)


def test_unknown_attention_long_impl_raises():
    stack = _stack()
    stack.attention_long_impl = "triton"
    with torch.no_grad():
        with pytest.raises(ValueError, match="attention_long_impl"):
            stack.hip_attention_active(OnDevice, 7, 7)
        with pytest.raises(ValueError, match="attention_long_impl"):
            stack(torch.randn(2, 7, 8))                                    # with attention_impl = "torch" too
    with pytest.raises(ValueError, match="attention_long_impl"):
        stack.hip_train_active(OnDevice, 7, None)


def test_attention_long_impl_defaults_to_torch_and_is_pushed_to_both_stacks():
    from retrieval_cases import tiny_batch
    m = tiny_model().eval()
    assert m.attention_long_impl == "torch"
    assert m.encoder.encoder.attention_long_impl == "torch" and m.t5_decoder.attention_long_impl == "torch"
    assert "attention_long_impl" not in m.state_dict()
    batch = tiny_batch()
    want = m(batch).loss
    m.attention_impl, m.attention_long_impl = "hip", "hip"
    got = m(batch).loss                                                   # host tensors: the operators, same bits
    assert m.encoder.encoder.attention_long_impl == "hip" and m.t5_decoder.attention_long_impl == "hip"
    assert torch.equal(got, want)
    m.attention_long_impl = "triton"
    with pytest.raises(ValueError, match="attention_long_impl"):
        m(batch)
