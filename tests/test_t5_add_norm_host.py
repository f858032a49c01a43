"""The fused residual + dropout + RMS norm ("add-norm": csrc/t5_add_norm.hip, rqhip_t5_add_norm_fwd / _bwd; norm_impl =
"hip") on the host: the argument checks of the C entry points, which all come before any HIP call, the supported widths,
the workspace query, the option on the stack and on the model, and the fall-back to the operators on host tensors.
No GPU needed."""
import pytest
import torch

from retrieval_cases import tiny_batch, tiny_model


def _fwd(l, *, N=8, d=64, p_in=0.0, p_out=0.0, eps=1e-6):
    # every data pointer stays null: they are checked last, so a call that passes every other check launches nothing
    return l.rqhip_t5_add_norm_fwd(None, None, None, N, d, eps, p_in, p_out, None, None, None, None, None)


def _bwd(l, *, N=8, d=64, p_in=0.0, p_out=0.0, **_):
    return l.rqhip_t5_add_norm_bwd(None, None, None, None, None, N, d, p_in, p_out, None, None, None, None, None, 0, None)


@pytest.mark.parametrize("call,name", [(_fwd, b"t5_add_norm_fwd"), (_bwd, b"t5_add_norm_bwd")])
def test_argument_checks_without_gpu(call, name):
    from rqhip import _lib
    l = _lib.lib()
    assert call(l, N=-1) == -1 and b"bad sizes" in l.rqhip_last_error() and name in l.rqhip_last_error()
    assert call(l, d=0) == -1
    for d in (2, 6, 1028, 2048):
        assert call(l, d=d) == -2 and b"multiples of 4" in l.rqhip_last_error() and name in l.rqhip_last_error()
    for kw in ({"p_in": 1.0}, {"p_out": 1.0}, {"p_in": -0.1}, {"p_out": float("nan")}, {"p_in": 2.0}):
        assert call(l, **kw) == -1 and b"0 <= p < 1" in l.rqhip_last_error()
    # fully valid sizes, null data: refused last, and by name
    assert call(l) == -1 and b"null pointer" in l.rqhip_last_error()
    assert call(l, p_in=0.1, p_out=0.5) == -1 and b"null pointer" in l.rqhip_last_error()
    assert call(l, N=0) == 0                                # nothing to do


def test_pointer_and_workspace_checks_without_gpu():
    """Host buffers stand in for device memory: every call below is refused before it could be dereferenced."""
    from rqhip import _lib
    l = _lib.lib()
    N, d = 8, 64
    buf = torch.zeros(N * d + 4)
    a = buf.data_ptr()
    assert a % 16 == 0
    # the seed is needed as soon as either probability is positive
    assert l.rqhip_t5_add_norm_fwd(None, a, a, N, d, 1e-6, 0.0, 0.1, None, a, a, a, None) == -1
    assert b"seed" in l.rqhip_last_error()
    assert l.rqhip_t5_add_norm_bwd(a, a, a, a, None, N, d, 0.1, 0.0, None, a, None, a, a, 1 << 20, None) == -1
    assert b"seed" in l.rqhip_last_error()
    # 16-byte alignment of what is read and written as float4
    assert l.rqhip_t5_add_norm_fwd(None, a + 4, a, N, d, 1e-6, 0.0, 0.0, None, a, a, a, None) == -1
    assert b"16-byte aligned" in l.rqhip_last_error()
    assert l.rqhip_t5_add_norm_bwd(a, a, a, a + 4, None, N, d, 0.0, 0.0, None, a, None, a, a, 1 << 20, None) == -1
    assert b"16-byte aligned" in l.rqhip_last_error()
    # a missing or short workspace
    need = l.rqhip_t5_add_norm_bwd_workspace_bytes(N, d)
    assert l.rqhip_t5_add_norm_bwd(a, a, a, a, None, N, d, 0.0, 0.0, None, a, None, a, None, need, None) == -1
    assert b"workspace" in l.rqhip_last_error()
    assert l.rqhip_t5_add_norm_bwd(a, a, a, a, None, N, d, 0.0, 0.0, None, a, None, a, a, need - 1, None) == -1
    assert b"workspace" in l.rqhip_last_error()
    assert l.rqhip_t5_add_norm_bwd(a, a, a, a, None, N, d, 0.0, 0.0, None, a, None, None, a, need, None) == -1   # no d_w
    assert b"null pointer" in l.rqhip_last_error()


def test_supported_widths_and_workspace():
    from rqhip import _lib, ops
    l = _lib.lib()
    for d in range(-4, 1100):
        want = d % 4 == 0 and 4 <= d <= 1024
        assert bool(l.rqhip_t5_add_norm_supported(d)) == want, d
    assert ops.t5_add_norm_supported(torch.float32, 384)
    for dtype in (torch.float16, torch.bfloat16, torch.float64):
        assert not ops.t5_add_norm_supported(dtype, 384)
    # one [d] block per 64 rows (include/rqhip.h): a function of (N, d) alone, the same on every call
    for d in (4, 384, 1024):
        assert l.rqhip_t5_add_norm_bwd_workspace_bytes(0, d) > 0
        for N, blocks in ((1, 1), (64, 1), (65, 2), (200, 4), (4096, 64), (5184, 81), (16384, 256), (16385, 129),
                          (1 << 20, 256)):
            assert l.rqhip_t5_add_norm_bwd_workspace_bytes(N, d) == blocks * d * 4, (N, d)
            assert l.rqhip_t5_add_norm_bwd_workspace_bytes(N, d) == l.rqhip_t5_add_norm_bwd_workspace_bytes(N, d)
    assert l.rqhip_t5_add_norm_bwd_workspace_bytes(-1, 64) == 0 and l.rqhip_t5_add_norm_bwd_workspace_bytes(8, 6) == 0


def test_wrappers_reject_host_tensors():
    from rqhip import ops
    from rqhip._lib import RqHipError
    y, w = torch.zeros(3, 8), torch.ones(8)
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.t5_add_norm_fwd(None, y, w, 1e-6)
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.t5_add_norm_bwd(y, torch.zeros(3), w, y, None)


def test_option_values_and_state_dict():
    from modules.t5 import NORM_IMPLS, T5Config, T5Stack
    assert NORM_IMPLS == ("torch", "hip")
    keys = sorted(tiny_model().state_dict())
    m = tiny_model().eval()
    assert m.norm_impl == "torch" and m.encoder.encoder.norm_impl == "torch" and m.t5_decoder.norm_impl == "torch"
    m.norm_impl = "hip"
    with torch.no_grad():
        m(tiny_batch())
    assert m.encoder.encoder.norm_impl == "hip" and m.t5_decoder.norm_impl == "hip"
    assert sorted(m.state_dict()) == keys
    m.norm_impl = "bogus"
    with pytest.raises(ValueError, match="norm_impl"):
        m(tiny_batch())
    stack = T5Stack(T5Config(16, d_model=8, num_heads=2, d_ff=8, num_layers=1)).eval()
    assert stack.norm_impl == "torch"
    stack.norm_impl = "bogus"
    with pytest.raises(ValueError, match="norm_impl"):
        stack(torch.randn(2, 3, 8))

    class OnDevice:                # hip_norm_active reads only these
        is_cuda, dtype = True, torch.float32

    stack.norm_impl = "hip"
    assert stack.hip_norm_active(OnDevice) and not stack.hip_norm_active(torch.zeros(2, 3, 8))
    OnDevice.dtype = torch.float16
    assert not stack.hip_norm_active(OnDevice)
    stack.norm_impl = "torch"
    OnDevice.dtype = torch.float32
    assert not stack.hip_norm_active(OnDevice)


@pytest.mark.parametrize("attention", ["torch", "hip", "hip_train"])
def test_hip_norm_on_host_tensors_is_the_operators(attention):
    m = tiny_model().eval()
    m.attention_impl = attention
    batch = tiny_batch()

    def run():
        m.zero_grad(set_to_none=True)
        out = m(batch)
        out.loss.backward()
        return out.loss.detach(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}

    want, want_g = run()
    m.norm_impl = "hip"
    got, got_g = run()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and sorted(got_g) == sorted(want_g) and len(got_g) > 10
    for n in want_g:
        assert torch.equal(got_g[n], want_g[n]), n
