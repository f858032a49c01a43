"""The fused semantic-id heads + cross-entropy (csrc/sid_head_loss.hip, rqhip_sid_head_loss_fwd / _bwd; head_impl =
"hip") on the host: the argument checks of the C entry points, which all come before any HIP call, the supported shapes,
the option on the model, and the fall-back to the operators on host tensors.  No GPU needed."""
import ctypes as C

import pytest
import torch

from retrieval_cases import tiny_batch, tiny_model


def _fwd(l, *, B=8, T=4, L=3, K=16, d=64, ld_xb=None, ld_xt=None, ld_t=None, x=None, w=None, rest=None):
    # by default every data pointer stays null: they are checked last, so a call that passes every other check launches
    # nothing
    ld_xt = d if ld_xt is None else ld_xt
    ld_xb = T * d if ld_xb is None else ld_xb
    ld_t = L + 1 if ld_t is None else ld_t
    return l.rqhip_sid_head_loss_fwd(x, ld_xb, ld_xt, w, rest, ld_t, B, T, L, K, d, rest, rest, rest, rest, rest, None)


def _bwd(l, *, B=8, T=4, L=3, K=16, d=64, ld_xb=None, ld_xt=None, ld_t=None, x=None, w=None, rest=None):
    ld_xt = d if ld_xt is None else ld_xt
    ld_xb = T * d if ld_xb is None else ld_xb
    ld_t = L + 1 if ld_t is None else ld_t
    return l.rqhip_sid_head_loss_bwd(x, ld_xb, ld_xt, w, rest, ld_t, rest, rest, rest, B, T, L, K, d, None, None, None)


@pytest.mark.parametrize("call,name", [(_fwd, b"sid_head_loss_fwd"), (_bwd, b"sid_head_loss_bwd")])
def test_argument_checks_without_gpu(call, name):
    from rqhip import _lib
    l = _lib.lib()
    for kw in ({"B": 0}, {"B": -1}, {"T": -1}, {"d": -4}, {"K": -1}, {"L": -1}):
        assert call(l, **kw) == -1 and b"bad sizes" in l.rqhip_last_error() and name in l.rqhip_last_error(), kw
    for kw in ({"d": 2}, {"d": 6}, {"d": 1028}, {"K": 0}, {"K": 1025}, {"L": 0}, {"L": 9, "T": 9, "ld_t": 9}):
        assert call(l, **kw) == -2 and b"are implemented" in l.rqhip_last_error() and name in l.rqhip_last_error(), kw
    assert call(l, T=2) == -1 and b"fewer than the L=3 levels" in l.rqhip_last_error() and name in l.rqhip_last_error()
    assert call(l, ld_t=2) == -1 and b"target row stride" in l.rqhip_last_error() and name in l.rqhip_last_error()
    for kw in ({"ld_xb": 4 * 64 + 2}, {"ld_xt": 65}, {"ld_xt": -64}):
        assert call(l, **kw) == -1 and b"x strides" in l.rqhip_last_error() and name in l.rqhip_last_error(), kw
    # fully valid sizes, null data: refused last, and by name
    assert call(l) == -1 and b"null pointer" in l.rqhip_last_error() and name in l.rqhip_last_error()
    assert call(l, T=3, ld_t=3, ld_xb=0, ld_xt=0) == -1 and b"null pointer" in l.rqhip_last_error()


@pytest.mark.parametrize("call,name", [(_fwd, b"sid_head_loss_fwd"), (_bwd, b"sid_head_loss_bwd")])
def test_pointer_checks_without_gpu(call, name):
    """Host buffers stand in for device memory: every call below is refused before it could be dereferenced."""
    from rqhip import _lib
    l = _lib.lib()
    buf = torch.zeros(8 * 4 * 64 + 4)
    a = buf.data_ptr()
    assert a % 16 == 0
    three = (C.c_void_p * 3)(a, a, a)
    # the weights are L pointers: the array and each entry are checked
    assert call(l, x=a, w=None, rest=a) == -1 and b"null pointer" in l.rqhip_last_error()
    assert call(l, x=a, w=(C.c_void_p * 3)(a, None, a), rest=a) == -1 and b"null pointer" in l.rqhip_last_error()
    assert call(l, x=a, w=three, rest=None) == -1 and b"null pointer" in l.rqhip_last_error()
    # 16-byte alignment of what is read as float4
    assert call(l, x=a + 4, w=three, rest=a) == -1
    assert b"x" in l.rqhip_last_error() and b"16-byte aligned" in l.rqhip_last_error() and name in l.rqhip_last_error()
    if call is _fwd:
        assert call(l, x=a, w=(C.c_void_p * 3)(a, a + 8, a), rest=a) == -1 and b"16-byte aligned" in l.rqhip_last_error()
    else:
        assert call(l, x=a, w=three, rest=a) == 0      # neither d_x nor d_w wanted: nothing to do, nothing launched


def test_supported_shapes():
    from rqhip import _lib, ops
    l = _lib.lib()

    def want(d, K, L):
        return d % 4 == 0 and 4 <= d <= 1024 and 1 <= K <= 1024 and 1 <= L <= 8

    for d in range(-4, 1100):
        for K, L in ((256, 3), (1, 1), (1024, 8), (0, 3), (1025, 3), (256, 0), (256, 9)):
            assert bool(l.rqhip_sid_head_loss_supported(d, K, L)) == want(d, K, L), (d, K, L)
    for K in range(-1, 1030):
        for d, L in ((384, 3), (4, 1), (1024, 8), (6, 3), (384, 9)):
            assert bool(l.rqhip_sid_head_loss_supported(d, K, L)) == want(d, K, L), (d, K, L)
    for L in range(-1, 10):
        for d, K in ((384, 256), (4, 1), (1024, 1024), (1028, 256), (384, 1025)):
            assert bool(l.rqhip_sid_head_loss_supported(d, K, L)) == want(d, K, L), (d, K, L)
    assert ops.sid_head_loss_supported(torch.float32, 384, 256, 3)
    for dtype in (torch.float16, torch.bfloat16, torch.float64):
        assert not ops.sid_head_loss_supported(dtype, 384, 256, 3)


def test_wrappers_reject_host_tensors():
    from rqhip import ops
    from rqhip._lib import RqHipError
    x, w, t = torch.zeros(2, 3, 8), [torch.zeros(4, 8)] * 2, torch.zeros(2, 3, dtype=torch.long)
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.sid_head_loss_fwd(x, w, t, 2)
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.sid_head_loss_bwd(x, w, t, torch.zeros(2, 2, 4), torch.zeros(2, 2), torch.ones(()), 2)


def test_option_values_and_state_dict():
    from modules.model import HEAD_IMPLS
    assert HEAD_IMPLS == ("torch", "hip")
    keys = sorted(tiny_model().state_dict())
    m = tiny_model().eval()
    assert m.head_impl == "torch"
    m.head_impl = "hip"
    with torch.no_grad():
        m(tiny_batch())
    assert sorted(m.state_dict()) == keys
    m.head_impl = "nope"
    with pytest.raises(ValueError, match="head_impl"):
        m(tiny_batch())

    class OnDevice:                # hip_head_active reads only these
        is_cuda, dtype, shape = True, torch.float32, (2, 4, 8)

    m.head_impl = "hip"
    assert m.hip_head_active(OnDevice) and not m.hip_head_active(torch.zeros(2, 4, 8))
    OnDevice.dtype = torch.float16
    assert not m.hip_head_active(OnDevice)
    OnDevice.dtype, OnDevice.shape = torch.float32, (2, 4, 6)
    assert not m.hip_head_active(OnDevice)
    OnDevice.shape = (2, 4, 8)
    m.head_impl = "torch"
    assert not m.hip_head_active(OnDevice)


@pytest.mark.parametrize("grad", [True, False])
def test_hip_head_on_host_tensors_is_the_operators(grad, monkeypatch):
    import modules.model as model_module
    calls = {"fwd": 0, "bwd": 0}

    def counted(name):
        def f(*a, **kw):
            calls[name] += 1
            raise AssertionError("the fused op was called on host tensors")
        return f

    monkeypatch.setattr(model_module.ops, "sid_head_loss_fwd", counted("fwd"))
    monkeypatch.setattr(model_module.ops, "sid_head_loss_bwd", counted("bwd"))
    m = tiny_model().eval()
    batch = tiny_batch()

    def run():
        m.zero_grad(set_to_none=True)
        with torch.set_grad_enabled(grad):
            out = m(batch)
        assert out.logits is None and out.loss.shape == () and out.loss_d.shape == (3,) and not out.loss_d.requires_grad
        grads = {}
        if grad:
            out.loss.backward()
            grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        return out.loss.detach(), out.loss_d, grads

    want, want_d, want_g = run()
    m.head_impl = "hip"
    got, got_d, got_g = run()
    assert calls == {"fwd": 0, "bwd": 0}
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(got_d.view(torch.int32), want_d.view(torch.int32))
    assert sorted(got_g) == sorted(want_g) and (len(got_g) > 10 or not grad)
    for n in want_g:
        assert torch.equal(got_g[n], want_g[n]), n
