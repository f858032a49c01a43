"""The fused T5 feed-forward (csrc/t5_ffn.hip, rqhip_t5_ffn_fwd / _bwd; ffn_impl = "hip") on the host: the argument checks
of the C entry points, which all come before any HIP call, the supported (d_model, d_ff), the workspace query, the option
on the stack and on the model, and the fall-back to the operators on host tensors.  No GPU needed."""
import pytest
import torch

from retrieval_cases import tiny_batch, tiny_model


def _fwd(l, *, N=8, d=64, F=96, p=0.0):
    # every data pointer stays null: they are checked last, so a call that passes every other check launches nothing
    return l.rqhip_t5_ffn_fwd(None, None, None, N, d, F, p, None, None, None, None)


def _bwd(l, *, N=8, d=64, F=96, p=0.0):
    # one output is wanted (a host address that is never dereferenced), or the call would have nothing to do
    want = _HOST.data_ptr()
    return l.rqhip_t5_ffn_bwd(None, None, None, None, None, N, d, F, p, None, want, None, None, None, None)


_HOST = torch.zeros(8 * 96 + 4)


@pytest.mark.parametrize("call,name", [(_fwd, b"t5_ffn_fwd"), (_bwd, b"t5_ffn_bwd")])
def test_argument_checks_without_gpu(call, name):
    from rqhip import _lib
    l = _lib.lib()
    for kw in ({"N": -1}, {"d": 0}, {"F": 0}, {"d": -32}):
        assert call(l, **kw) == -1 and b"bad sizes" in l.rqhip_last_error() and name in l.rqhip_last_error()
    for kw in ({"d": 30}, {"d": 48}, {"F": 30}, {"F": 48}, {"d": 16}, {"d": 544}, {"F": 8224}, {"d": 1024}):
        assert call(l, **kw) == -2 and b"multiples of 32" in l.rqhip_last_error() and name in l.rqhip_last_error()
    for p in (1.0, -0.1, float("nan"), 2.0):
        assert call(l, p=p) == -1 and b"0 <= p < 1" in l.rqhip_last_error() and name in l.rqhip_last_error()
    # fully valid sizes, null data: refused last, and by name
    assert call(l) == -1 and b"null pointer" in l.rqhip_last_error() and name in l.rqhip_last_error()
    assert call(l, p=0.5) == -1 and b"null pointer" in l.rqhip_last_error()
    assert call(l, N=0) == 0                                # nothing to do
    assert call(l, N=0, p=0.5) == 0
    assert call(l, N=0, d=48) == -2                         # but still a shape the kernels do not take


def test_pointer_checks_without_gpu():
    """Host buffers stand in for device memory: every call below is refused before it could be dereferenced."""
    from rqhip import _lib
    l = _lib.lib()
    N, d, F = 8, 64, 96
    a = _HOST.data_ptr()
    assert a % 16 == 0
    # nothing wanted: nothing to do, whatever else is passed
    assert l.rqhip_t5_ffn_bwd(None, None, None, None, None, N, d, F, 0.0, None, None, None, None, None, None) == 0
    assert l.rqhip_t5_ffn_bwd(a, a, a, a, a, N, d, F, 0.5, None, None, None, None, None, None) == 0
    # the seed is needed as soon as p is positive
    assert l.rqhip_t5_ffn_fwd(a, a, a, N, d, F, 0.1, None, a, a, None) == -1
    assert b"seed" in l.rqhip_last_error() and b"t5_ffn_fwd" in l.rqhip_last_error()
    assert l.rqhip_t5_ffn_bwd(a, a, a, a, a, N, d, F, 0.1, None, a, None, None, None, None) == -1
    assert b"seed" in l.rqhip_last_error() and b"t5_ffn_bwd" in l.rqhip_last_error()
    # d_wi needs the workspace that holds g
    assert l.rqhip_t5_ffn_bwd(a, a, a, a, a, N, d, F, 0.0, None, None, a, None, None, None) == -3
    assert b"workspace" in l.rqhip_last_error() and b"t5_ffn_bwd" in l.rqhip_last_error()
    # 16-byte alignment of everything that is read or written as vectors
    for k in range(5):
        args = [a, a, a, a, a]
        args[k] = a + 4
        if k != 3:
            assert l.rqhip_t5_ffn_fwd(*(args[:3]), N, d, F, 0.0, None, args[4], a, None) == -1
            assert b"16-byte aligned" in l.rqhip_last_error() and b"t5_ffn_fwd" in l.rqhip_last_error()
        assert l.rqhip_t5_ffn_bwd(*args, N, d, F, 0.0, None, a, a, a, a, None) == -1
        assert b"16-byte aligned" in l.rqhip_last_error() and b"t5_ffn_bwd" in l.rqhip_last_error()
    assert l.rqhip_t5_ffn_fwd(a, a, a, N, d, F, 0.0, None, a, a + 8, None) == -1        # h
    assert b"16-byte aligned" in l.rqhip_last_error()
    for k in range(4):                                                                   # d_x, d_wi, d_wo, workspace
        outs = [a, a, a, a]
        outs[k] = a + 4
        assert l.rqhip_t5_ffn_bwd(a, a, a, a, a, N, d, F, 0.0, None, *outs, None) == -1
        assert b"16-byte aligned" in l.rqhip_last_error()
    # a null input next to wanted outputs
    for k in range(5):
        args = [a, a, a, a, a]
        args[k] = None
        assert l.rqhip_t5_ffn_bwd(*args, N, d, F, 0.0, None, a, a, a, a, None) == -1
        assert b"null pointer" in l.rqhip_last_error()
    assert l.rqhip_t5_ffn_fwd(a, a, a, N, d, F, 0.0, None, None, a, None) == -1           # no y
    assert b"null pointer" in l.rqhip_last_error()


def test_supported_shapes_and_workspace():
    from rqhip import _lib, ops
    l = _lib.lib()

    def rule(d, F):        # include/rqhip.h: multiples of 32, 32 <= d <= 512, 32 <= F <= 8192
        return d % 32 == 0 and 32 <= d <= 512 and F % 32 == 0 and 32 <= F <= 8192

    for d in list(range(-32, 600)) + [1024]:
        for F in (-32, 0, 16, 30, 32, 48, 64, 96, 100, 1024, 2048, 8192, 8193, 8224, 16384):
            assert bool(l.rqhip_t5_ffn_supported(d, F)) == rule(d, F), (d, F)
    for F in range(0, 8300, 4):
        assert bool(l.rqhip_t5_ffn_supported(384, F)) == rule(384, F), F
    for d in (32, 64, 128, 384, 512):
        for F in (32, 96, 256, 1024, 2048):
            assert ops.t5_ffn_supported(torch.float32, d, F)
    for dtype in (torch.float16, torch.bfloat16, torch.float64):
        assert not ops.t5_ffn_supported(dtype, 384, 1024)
    # exactly the g buffer
    for N in (0, 1, 17, 256, 5184, 1 << 20):
        for d, F in ((32, 32), (384, 1024), (512, 8192)):
            assert l.rqhip_t5_ffn_bwd_workspace_bytes(N, d, F) == 4 * N * F
    assert l.rqhip_t5_ffn_bwd_workspace_bytes(-1, 64, 96) == 0 and l.rqhip_t5_ffn_bwd_workspace_bytes(8, 48, 96) == 0


def test_wrappers_reject_host_tensors_and_other_dtypes():
    from rqhip import ops
    from rqhip._lib import RqHipError
    x, wi, wo = torch.zeros(3, 32), torch.zeros(64, 32), torch.zeros(32, 64)
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.t5_ffn_fwd(x, wi, wo)
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.t5_ffn_bwd(x, wi, wo, torch.zeros(3, 64), x)


def test_option_values_and_state_dict():
    from modules.t5 import FFN_IMPLS, T5Config, T5Stack
    assert FFN_IMPLS == ("torch", "hip")
    keys = sorted(tiny_model(32, 32).state_dict())
    m = tiny_model(32, 32).eval()
    assert m.ffn_impl == "torch" and m.encoder.encoder.ffn_impl == "torch" and m.t5_decoder.ffn_impl == "torch"
    m.ffn_impl = "hip"
    with torch.no_grad():
        m(tiny_batch())
    assert m.encoder.encoder.ffn_impl == "hip" and m.t5_decoder.ffn_impl == "hip"
    assert sorted(m.state_dict()) == keys
    for norm in ("torch", "hip"):
        m.ffn_impl, m.norm_impl = "bogus", norm
        with pytest.raises(ValueError, match="ffn_impl"):
            m(tiny_batch())
    stack = T5Stack(T5Config(16, d_model=32, num_heads=2, d_ff=64, num_layers=1)).eval()
    assert stack.ffn_impl == "torch"
    stack.ffn_impl = "bogus"
    with pytest.raises(ValueError, match="ffn_impl"):
        stack(torch.randn(2, 3, 32))

    class OnDevice:                # hip_ffn_active reads only these
        is_cuda, dtype = True, torch.float32

    stack.ffn_impl = "hip"
    assert stack.hip_ffn_active(OnDevice) and not stack.hip_ffn_active(torch.zeros(2, 3, 32))
    for dtype in (torch.float16, torch.bfloat16, torch.float64):
        OnDevice.dtype = dtype
        assert not stack.hip_ffn_active(OnDevice)
    OnDevice.dtype = torch.float32
    stack.train()
    assert stack.hip_ffn_active(OnDevice)          # train mode too
    stack.ffn_impl = "torch"
    assert not stack.hip_ffn_active(OnDevice)
    narrow = T5Stack(T5Config(16, d_model=32, num_heads=2, d_ff=40, num_layers=1))
    narrow.ffn_impl = "hip"
    assert not narrow.hip_ffn_active(OnDevice)      # a d_ff the kernel does not take: the operators


@pytest.mark.parametrize("attention,norm", [("torch", "torch"), ("hip_train", "torch"), ("torch", "hip"), ("hip", "hip")])
def test_hip_ffn_on_host_tensors_is_the_operators(attention, norm, monkeypatch):
    import modules.t5 as t5_module

    def refuse(*a, **kw):
        raise AssertionError("the fused op was called on host tensors")

    monkeypatch.setattr(t5_module.ops, "t5_ffn_fwd", refuse)
    monkeypatch.setattr(t5_module.ops, "t5_ffn_bwd", refuse)
    monkeypatch.setattr(t5_module.T5FFNFunction, "apply", refuse)
    m = tiny_model(32, 32).eval()
    m.attention_impl, m.norm_impl = attention, norm
    batch = tiny_batch()

    def run():
        m.zero_grad(set_to_none=True)
        out = m(batch)
        out.loss.backward()
        return out.loss.detach(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}

    want, want_g = run()
    m.ffn_impl = "hip"
    got, got_g = run()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and sorted(got_g) == sorted(want_g) and len(got_g) > 10
    for n in want_g:
        assert torch.equal(got_g[n], want_g[n]), n
