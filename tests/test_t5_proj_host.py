"""The grouped T5 attention projections (csrc/t5_proj.hip, rqhip_t5_proj_fwd / _bwd; proj_impl = "hip") on the host: the
supported shapes, the argument checks of the C entry points, which all come before any HIP call, the option on the stack
and on the model, and the fall-back to the operators on host tensors.  No GPU needed."""
import ctypes as C

import pytest
import torch

from retrieval_cases import tiny_batch, tiny_model

_HOST = torch.zeros(8 * 96 + 8)      # host memory that stands in for device memory: never dereferenced
N, D_IN, D_OUT = 8, 64, 96


def _ptrs(values):
    return (C.c_void_p * len(values))(*values)


def _lds(values):
    return (C.c_int64 * len(values))(*values)


def _fwd(l, *, x="a", ld_x=D_IN, w="a", y="a", ld_y=D_OUT, n=3, N=N, d_in=D_IN, d_out=D_OUT):
    """rqhip_t5_proj_fwd with every pointer valid and aligned unless replaced: "a" the host buffer, None a null, a list the
    array's entries, an int every entry."""
    a = _HOST.data_ptr()
    m = max(n, 1)
    arr = lambda v: None if v is None else _ptrs(v if isinstance(v, list) else [a if v == "a" else v] * m)
    lds = None if ld_y is None else _lds(ld_y if isinstance(ld_y, list) else [ld_y] * m)
    return l.rqhip_t5_proj_fwd(a if x == "a" else x, ld_x, arr(w), arr(y), lds, n, N, d_in, d_out, None)


def _bwd(l, *, x="a", ld_x=D_IN, w="a", d_y="a", ld_dy=D_OUT, n=3, N=N, d_in=D_IN, d_out=D_OUT, d_x="a", d_w="a"):
    a = _HOST.data_ptr()
    m = max(n, 1)
    arr = lambda v: None if v is None else _ptrs(v if isinstance(v, list) else [a if v == "a" else v] * m)
    lds = None if ld_dy is None else _lds(ld_dy if isinstance(ld_dy, list) else [ld_dy] * m)
    return l.rqhip_t5_proj_bwd(a if x == "a" else x, ld_x, arr(w), arr(d_y), lds, n, N, d_in, d_out,
                               a if d_x == "a" else d_x, arr(d_w), None)


def test_supported_table():
    from rqhip import _lib, ops
    l = _lib.lib()

    def rule(d_in, d_out, n):        # include/rqhip.h: multiples of 32 in 32 .. 512, 1 <= n <= 8
        return d_in % 32 == 0 and 32 <= d_in <= 512 and d_out % 32 == 0 and 32 <= d_out <= 512 and 1 <= n <= 8

    widths = (-32, 0, 16, 31, 32, 33, 48, 64, 100, 384, 480, 512, 513, 544, 1024)
    for d_in in widths:
        for d_out in widths:
            for n in (-1, 0, 1, 2, 3, 8, 9, 16):
                assert bool(l.rqhip_t5_proj_supported(d_in, d_out, n)) == rule(d_in, d_out, n), (d_in, d_out, n)
    for d in range(0, 600):
        assert bool(l.rqhip_t5_proj_supported(d, 384, 3)) == rule(d, 384, 3), d
        assert bool(l.rqhip_t5_proj_supported(384, d, 1)) == rule(384, d, 1), d
    for d_in, d_out in ((128, 384), (384, 128), (384, 384), (512, 512), (64, 128)):
        assert ops.t5_proj_supported(torch.float32, d_in, d_out) and ops.t5_proj_supported(torch.float32, d_in, d_out, 8)
        assert not ops.t5_proj_supported(torch.float32, d_in, d_out, 9)
    for dtype in (torch.float16, torch.bfloat16, torch.float64):
        assert not ops.t5_proj_supported(dtype, 384, 384, 3)
    assert ops.T5_PROJ_MAX_GROUP == 8


@pytest.mark.parametrize("call,name", [(_fwd, b"t5_proj_fwd"), (_bwd, b"t5_proj_bwd")])
def test_size_and_shape_checks_without_gpu(call, name):
    from rqhip import _lib
    l = _lib.lib()
    for kw in ({"N": -1}, {"d_in": 0}, {"d_out": 0}, {"d_in": -32}, {"n": -1}):
        assert call(l, **kw) == -1 and b"bad sizes" in l.rqhip_last_error() and name in l.rqhip_last_error(), kw
    for kw in ({"d_in": 31}, {"d_in": 48}, {"d_in": 544}, {"d_out": 31}, {"d_out": 48}, {"d_out": 544}, {"n": 0},
               {"n": 9}):
        assert call(l, **kw) == -2 and b"multiples of 32" in l.rqhip_last_error() and name in l.rqhip_last_error(), kw
    assert call(l, N=0) == 0                                 # nothing to do
    assert call(l, N=0, x=None, w=None) == 0                 # ... whatever the pointers are
    assert call(l, N=0, d_in=48) == -2                       # but still a shape the kernels do not take
    assert call(l, N=0, n=9) == -2


def test_forward_pointer_checks_without_gpu():
    from rqhip import _lib
    l = _lib.lib()
    a = _HOST.data_ptr()
    assert a % 16 == 0
    for kw in ({"x": None}, {"w": None}, {"y": None}, {"ld_y": None}, {"w": [a, None, a]}, {"y": [a, a, None]}):
        assert _fwd(l, **kw) == -1 and b"null pointer" in l.rqhip_last_error() and b"t5_proj_fwd" in l.rqhip_last_error(), kw
    assert _fwd(l, ld_y=[D_OUT, D_OUT - 1, D_OUT]) == -1
    assert b"ld_y[1]=95 is less than d_out=96" in l.rqhip_last_error() and b"t5_proj_fwd" in l.rqhip_last_error()
    assert _fwd(l, ld_y=[D_OUT, 4 * D_OUT, 0]) == -1 and b"ld_y[2]=0" in l.rqhip_last_error()
    for kw in ({"ld_x": D_IN - 4}, {"ld_x": D_IN + 2}, {"x": a + 4}):
        assert _fwd(l, **kw) == -1 and b"x must be 16-byte aligned" in l.rqhip_last_error(), kw
    assert _fwd(l, w=[a, a + 4, a]) == -1 and b"w[1] must be 16-byte aligned" in l.rqhip_last_error()
    assert _fwd(l, y=[a, a, a + 2]) == -1 and b"y[2] 4-byte aligned" in l.rqhip_last_error()


def test_backward_pointer_checks_without_gpu():
    from rqhip import _lib
    l = _lib.lib()
    a = _HOST.data_ptr()
    for kw in ({"x": None}, {"w": None}, {"d_y": None}, {"ld_dy": None}, {"w": [a, None, a]}):
        assert _bwd(l, **kw) == -1 and b"null pointer" in l.rqhip_last_error() and b"t5_proj_bwd" in l.rqhip_last_error(), kw
    assert _bwd(l, ld_dy=[D_OUT, D_OUT - 4, D_OUT]) == -1
    assert b"ld_dy[1]=92 >= d_out=96" in l.rqhip_last_error() and b"t5_proj_bwd" in l.rqhip_last_error()
    assert _bwd(l, ld_dy=[D_OUT + 2, D_OUT, D_OUT]) == -1 and b"ld_dy[0]=98" in l.rqhip_last_error()
    assert _bwd(l, d_y=[a, a, a + 4]) == -1 and b"d_y[2] and w[2] must be 16-byte aligned" in l.rqhip_last_error()
    assert _bwd(l, w=[a + 8, a, a]) == -1 and b"d_y[0] and w[0] must be 16-byte aligned" in l.rqhip_last_error()
    for kw in ({"ld_x": D_IN - 4}, {"ld_x": D_IN + 1}, {"x": a + 4}, {"d_x": a + 8}):
        assert _bwd(l, **kw) == -1 and b"x and d_x must be 16-byte aligned" in l.rqhip_last_error(), kw
    assert _bwd(l, d_w=[a, a + 2, None]) == -1 and b"d_w[1] must be 4-byte aligned" in l.rqhip_last_error()
    # nothing wanted, or no upstream gradient at all: nothing is launched
    assert _bwd(l, d_x=None, d_w=None) == 0
    assert _bwd(l, d_x=None, d_w=[None, None, None]) == 0
    assert _bwd(l, d_y=[None, None, None]) == 0
    # a missing d_y[j] takes its ld_dy[j] and its d_w[j] out of the checks
    assert _bwd(l, d_y=[None, None, None], ld_dy=[0, 1, 2], d_w=[a + 2, a + 2, a + 2]) == 0


def test_wrappers_reject_host_tensors():
    from rqhip import ops
    from rqhip._lib import RqHipError
    x, w = torch.zeros(3, 32), torch.zeros(64, 32)
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.t5_proj_fwd(x, [w, w])
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.t5_proj_bwd(x, [w], [torch.zeros(3, 64)])


def test_option_values_and_state_dict():
    from modules.t5 import PROJ_IMPLS, T5Config, T5Stack
    assert PROJ_IMPLS == ("torch", "hip")
    keys = sorted(tiny_model(32, 32).state_dict())
    m = tiny_model(32, 32).eval()
    assert m.proj_impl == "torch" and m.encoder.encoder.proj_impl == "torch" and m.t5_decoder.proj_impl == "torch"
    m.proj_impl = "hip"
    with torch.no_grad():
        m(tiny_batch())
    assert m.encoder.encoder.proj_impl == "hip" and m.t5_decoder.proj_impl == "hip"
    assert sorted(m.state_dict()) == keys
    for attention in ("torch", "hip_train"):
        m.proj_impl, m.attention_impl = "bogus", attention
        with pytest.raises(ValueError, match="proj_impl"):
            m(tiny_batch())
    stack = T5Stack(T5Config(16, d_model=32, num_heads=2, d_ff=64, num_layers=1)).eval()
    assert stack.proj_impl == "torch"
    stack.proj_impl = "bogus"
    with pytest.raises(ValueError, match="proj_impl"):
        stack(torch.randn(2, 3, 32))
    decoder = T5Stack(T5Config(16, d_model=32, num_heads=2, d_ff=64, num_layers=1, is_decoder=True)).eval()
    assert len(decoder.cross_kv(torch.randn(2, 3, 32))) == 1
    decoder.proj_impl = "bogus"
    with pytest.raises(ValueError, match="proj_impl"):
        decoder.cross_kv(torch.randn(2, 3, 32))

    class OnDevice:                # hip_proj_active reads only these of x
        is_cuda, dtype = True, torch.float32

    stack.proj_impl = "hip"
    assert not stack.hip_proj_active(torch.zeros(2, 3, 32))      # host tensors
    assert not stack.hip_proj_active(OnDevice)                   # host weights
    stack.proj_impl = "torch"
    assert not stack.hip_proj_active(OnDevice)


@pytest.mark.parametrize("attention,norm", [("torch", "torch"), ("hip_train", "torch"), ("torch", "hip"), ("hip", "hip")])
def test_hip_proj_on_host_tensors_is_the_operators(attention, norm, monkeypatch):
    import modules.t5 as t5_module

    def refuse(*a, **kw):
        raise AssertionError("the fused op was called on host tensors")

    monkeypatch.setattr(t5_module.ops, "t5_proj_fwd", refuse)
    monkeypatch.setattr(t5_module.ops, "t5_proj_bwd", refuse)
    monkeypatch.setattr(t5_module.T5ProjFunction, "apply", refuse)
    m = tiny_model(32, 32).eval()
    m.attention_impl, m.norm_impl = attention, norm
    batch = tiny_batch()

    def run():
        m.zero_grad(set_to_none=True)
        out = m(batch)
        out.loss.backward()
        return out.loss.detach(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}

    want, want_g = run()
    m.proj_impl = "hip"
    got, got_g = run()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and sorted(got_g) == sorted(want_g) and len(got_g) > 10
    for n in want_g:
        assert torch.equal(got_g[n], want_g[n]), n
