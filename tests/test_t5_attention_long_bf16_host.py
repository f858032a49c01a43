"""The "bf16" arithmetic of the long fused T5 attention on the host (rqhip_t5_attention_long_*_bf16, the `arith` keyword of
ops.t5_attention_long*, the trailing `arith` of autograd.T5AttentionLongFunction, the `attention_arith` attribute of the stacks and the
model): the argument checks of the three new C entry points (their twins', under their own names), the keyword's default
and validation, and the attribute's default, validation and lack of effect on host tensors.  No GPU needed."""
import inspect

import pytest
import torch

from retrieval_cases import tiny_batch, tiny_model

OK_PTR = 4096      # a non-null, 16-byte aligned address that is never dereferenced: every check below fails before a launch
ODD_PTR = 4096 + 8
FWD, TRAIN, BWD = "t5_attention_long_bf16", "t5_attention_long_fwd_train_bf16", "t5_attention_long_bwd_bf16"


def _fwd(l, *, ptr=OK_PTR, R=4, Rk=4, H=6, d_kv=64, Tq=300, Tk=300, ld=None, past=0, anc=None, bias=None, n_delta=0,
         offset=0, causal=0):
    ld = H * 64 if ld is None else ld
    return l.rqhip_t5_attention_long_bf16(ptr, ld, OK_PTR, OK_PTR, ld, R, Rk, H, d_kv, Tq, Tk, bias, n_delta, offset,
                                          None, causal, past, anc, OK_PTR, ld, None)


def _train(l, *, ptr=OK_PTR, R=4, Rk=4, H=6, Tq=300, Tk=300, ld=None, bias=None, n_delta=0, offset=0, causal=0, p=0.0):
    ld = H * 64 if ld is None else ld
    return l.rqhip_t5_attention_long_fwd_train_bf16(ptr, ld, OK_PTR, OK_PTR, ld, R, Rk, H, 64, Tq, Tk, bias, n_delta,
                                                    offset, None, causal, p, None, OK_PTR, ld, OK_PTR, OK_PTR, None)


def _bwd(l, *, ptr=OK_PTR, R=4, Rk=4, H=6, Tq=300, Tk=300, ld=None, bias=None, n_delta=0, offset=0, causal=0, ws=OK_PTR,
         ws_bytes=None):
    ld = H * 64 if ld is None else ld
    if ws_bytes is None:
        ws_bytes = l.rqhip_t5_attention_long_bwd_workspace_bytes(R, H, Tq, Tk)
    return l.rqhip_t5_attention_long_bwd_bf16(ptr, ld, OK_PTR, OK_PTR, ld, OK_PTR, ld, OK_PTR, OK_PTR, OK_PTR, ld, R, Rk,
                                              H, 64, Tq, Tk, bias, n_delta, offset, None, causal, 0.0, None, OK_PTR,
                                              OK_PTR, OK_PTR, OK_PTR if bias else None, ws, ws_bytes, None)


NAMED = ((_fwd, FWD), (_train, TRAIN), (_bwd, BWD))


def test_bf16_entry_points_fail_their_twins_checks_under_their_own_names():
    from rqhip import _lib
    l = _lib.lib()

    def err():
        return l.rqhip_last_error()

    def named(name):           # the message names THIS entry point, not its fp32 twin
        return err().startswith(name.encode() + b":")

    # dense K/V at past = 0 only
    assert _fwd(l, past=1) == -2 and b"past = 0" in err() and named(FWD)
    assert _fwd(l, anc=OK_PTR) == -2 and b"ancestor" in err() and named(FWD)
    # the limits
    assert _fwd(l, Tk=2049) == -2 and b"<= 2048" in err() and named(FWD)
    assert _fwd(l, Tq=2049, Tk=2048) == -2 and b"<= 2048" in err()
    assert _train(l, Tk=2049) == -2 and b"<= 2048" in err() and named(TRAIN)
    assert _bwd(l, Tk=2049) == -2 and b"<= 2048" in err() and named(BWD)
    assert _fwd(l, d_kv=32) == -2 and b"d_kv = 64" in err() and named(FWD)
    assert _fwd(l, H=0) == -1 and _fwd(l, Tq=0) == -1 and _fwd(l, Tk=0) == -1
    assert _fwd(l, R=10, Rk=4) == -1 and b"multiple" in err() and named(FWD)
    # pointers: null, then misaligned
    for call, name in NAMED:
        assert call(l, ptr=None) == -1 and b"null pointer" in err() and named(name)
        assert call(l, ptr=ODD_PTR) == -1 and b"16-byte aligned" in err() and named(name)
    assert _train(l, p=0.5) == -1 and b"seed" in err() and named(TRAIN)          # dropout without a seed
    assert _bwd(l, ws=ODD_PTR) == -1 and b"16-byte aligned" in err() and named(BWD)
    for call, name in NAMED:
        # strides
        assert call(l, ld=6 * 64 + 2) == -1 and b"multiples of 4" in err() and named(name)
        assert call(l, ld=6 * 64 - 4) == -1 and b"H * 64" in err() and named(name)
        # Tq > Tk goes with neither causal nor a bias table
        assert call(l, Tq=300, Tk=299, causal=1) == -1 and b"exceeds Tk" in err() and named(name)
        assert call(l, Tq=300, Tk=299, bias=OK_PTR, n_delta=598, offset=299) == -1 and b"exceeds Tk" in err()
        # the bias table must cover every delta of the call
        assert call(l, bias=OK_PTR, n_delta=598, offset=299) == -1 and b"bias table" in err() and named(name)
        assert call(l, bias=OK_PTR, n_delta=599, offset=298) == -1 and b"bias table" in err()
    # the training pair takes one K/V per row
    assert _train(l, R=4, Rk=2) == -2 and b"Rk = R" in err() and named(TRAIN)
    assert _bwd(l, R=4, Rk=2) == -2 and b"Rk = R" in err() and named(BWD)
    # the workspace: the fp32 arm's size
    need = l.rqhip_t5_attention_long_bwd_workspace_bytes(4, 6, 300, 300)
    assert _bwd(l, ws_bytes=need - 1) == -1 and b"workspace" in err() and str(need).encode() in err() and named(BWD)
    assert _bwd(l, ws=None) == -1 and b"null pointer" in err()
    # nothing to do
    assert _fwd(l, R=0, Rk=0) == 0 and _train(l, R=0, Rk=0) == 0 and _bwd(l, R=0, Rk=0) == 0


def test_the_new_symbols_have_their_twins_signatures():
    from rqhip import _lib
    for twin in ("rqhip_t5_attention_long", "rqhip_t5_attention_long_fwd_train", "rqhip_t5_attention_long_bwd"):
        assert _lib.SIGNATURES[twin + "_bf16"] == _lib.SIGNATURES[twin]
    assert _lib.lib().rqhip_version() == 462


def test_arith_defaults_to_fp32_and_unknown_values_raise_before_any_other_check():
    from rqhip import autograd, ops
    from rqhip._lib import RqHipError
    for fn in (ops.t5_attention_long, ops.t5_attention_long_fwd_train, ops.t5_attention_long_bwd):
        par = inspect.signature(fn).parameters["arith"]
        assert par.default == "fp32" and par.kind is inspect.Parameter.KEYWORD_ONLY
    junk = object()             # not a tensor: any other check would trip over it first
    with pytest.raises(RqHipError, match="t5_attention_long: arith must be one of"):
        ops.t5_attention_long(junk, junk, junk, 6, arith="fp16")
    with pytest.raises(RqHipError, match="t5_attention_long_fwd_train: arith must be one of"):
        ops.t5_attention_long_fwd_train(junk, junk, junk, 6, arith="tf32")
    with pytest.raises(RqHipError, match="t5_attention_long_bwd: arith must be one of"):
        ops.t5_attention_long_bwd(junk, junk, junk, junk, junk, junk, junk, 6, arith=None)
    # the one Function takes the arithmetic as its trailing argument, "fp32" without it, and hands it to the ops
    call = (junk, junk, junk, None, 6, 0, None, False, 0.0, None)
    with pytest.raises(RqHipError, match="t5_attention_long_fwd_train: arith must be one of"):
        autograd.T5AttentionLongFunction.apply(*call, "fp16")
    params = list(inspect.signature(autograd.T5AttentionLongFunction.forward).parameters.values())
    assert params[-1].name == "arith" and params[-1].default == "fp32" and len(params) == 1 + len(call) + 1
    for arith in ("fp32", "bf16"):      # a known one goes on to the next check, which trips over the junk
        with pytest.raises(Exception) as info:
            autograd.T5AttentionLongFunction.apply(*call, arith)
        assert "arith must be one of" not in str(info.value)


def test_a_host_tensor_is_refused_after_the_arithmetic_is_resolved():
    from rqhip import ops
    from rqhip._lib import RqHipError
    x = torch.zeros(1, 4, 64)
    with pytest.raises(RqHipError) as info:
        ops.t5_attention_long(x, x, x, 1, arith="bf16")
    assert "arith" not in str(info.value)


def _stack(is_decoder=False):
    from modules.t5 import T5Config, T5Stack
    return T5Stack(T5Config(16, d_model=8, num_heads=2, d_ff=8, num_layers=1, is_decoder=is_decoder)).eval()


def test_attention_arith_of_a_stack_defaults_to_fp32_and_is_validated_on_every_path():
    from modules import t5
    assert t5.ATTENTION_ARITHS == ("fp32", "bf16")
    stack = _stack()
    assert stack.attention_arith == "fp32" and stack.attention_arithmetic() == "fp32"
    x = torch.randn(2, 7, 8)
    with torch.no_grad():
        want = stack(x)
        stack.attention_arith = "bf16"
        assert stack.attention_arithmetic() == "bf16"
        assert torch.equal(stack(x), want)                                 # host tensors: the operators, same bits
        stack.attention_impl, stack.attention_long_impl = "hip", "hip"
        assert torch.equal(stack(x), want)
        stack.attention_impl, stack.attention_long_impl = "torch", "torch"
        stack.attention_arith = "fp16"
        with pytest.raises(ValueError, match="attention_arith"):
            stack(x)                                                        # with attention_impl = "torch" too
        with pytest.raises(ValueError, match="attention_arith"):
            stack.attention_arithmetic()


def test_attention_arith_of_the_model_is_pushed_to_both_stacks_and_leaves_matmul_arith_alone():
    m = tiny_model().eval()
    assert m.attention_arith == "fp32"
    assert m.encoder.encoder.attention_arith == "fp32" and m.t5_decoder.attention_arith == "fp32"
    batch = tiny_batch()
    want, keys = m(batch).loss, list(m.state_dict())
    m.attention_impl, m.attention_long_impl, m.attention_arith = "hip_train", "hip", "bf16"
    got = m(batch).loss                                                    # host tensors: the operators, same bits
    assert m.encoder.encoder.attention_arith == "bf16" and m.t5_decoder.attention_arith == "bf16"
    assert torch.equal(got, want) and list(m.state_dict()) == keys and "attention_arith" not in m.state_dict()
    assert m.matmul_arith == "fp32"
    assert m.encoder.encoder.matmul_arith == "fp32" and m.t5_decoder.matmul_arith == "fp32"
    m.matmul_arith, m.attention_arith = "bf16", "fp32"
    m(batch)
    assert m.encoder.encoder.attention_arith == "fp32" and m.encoder.encoder.matmul_arith == "bf16"
    m.attention_arith = "fp16"
    with pytest.raises(ValueError, match="attention_arith"):
        m(batch)
