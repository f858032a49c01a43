"""bf16 weight images on the host: the new C entry points (exported, declared, bound; every argument check before any HIP
call, with host buffers standing in for device memory as in tests/test_t5_bf16_host.py), the `w_images` keyword of the
ops, `weight_images` on the stack and on the model, and the holder's staleness key on CPU tensors.  No GPU needed."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT
from retrieval_cases import tiny_batch, tiny_model

TWINS = ("rqhip_t5_ffn_fwd", "rqhip_t5_ffn_bwd", "rqhip_t5_proj_fwd", "rqhip_t5_proj_bwd")
IMAGE_CALLS = ("rqhip_bf16_images", "rqhip_bf16_images_job_bytes", "rqhip_bf16_images_fill_jobs")
_HOST = torch.zeros(8 * 96 + 64)
_JOBS = torch.zeros(4096, dtype=torch.uint8)


def test_symbols_are_exported_declared_and_bound():
    from rqhip import _lib
    handle = ctypes.CDLL(_lib.SO_PATH)
    text = open(os.path.join(ROOT, "include", "rqhip.h")).read()
    declared = set(re.findall(r"\b(rqhip_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    for name in IMAGE_CALLS + tuple(t + "_bf16w" for t in TWINS):
        assert hasattr(handle, name) and name in declared and name in _lib.SIGNATURES, name
    for t in TWINS:      # the signatures of their _bf16 twins
        assert _lib.SIGNATURES[t + "_bf16w"] == _lib.SIGNATURES[t + "_bf16"], t
    assert _lib.lib().rqhip_version() == 462
    assert 'results are those of `*_bf16` on the weights the images were made from' in text


def _fill(l, *, src=None, img=None, img_t=None, rows=(32,), cols=(64,), n=None, host=None, tiles=True):
    a = _HOST.data_ptr()
    n = len(rows) if n is None else n
    vp = ctypes.c_void_p * max(n, 1)
    src = vp(*([a] * n)) if src is None else src
    img = vp(*([a] * n)) if img is None else img
    out = ctypes.c_int64(-5)
    rc = l.rqhip_bf16_images_fill_jobs(_JOBS.data_ptr() if host is None else host, src, img, img_t,
                                       (ctypes.c_int64 * max(n, 1))(*rows), (ctypes.c_int64 * max(n, 1))(*cols), n,
                                       ctypes.byref(out) if tiles else None)
    return rc, out.value


def test_image_job_table_checks_without_gpu():
    from rqhip import _lib
    l = _lib.lib()
    a = _HOST.data_ptr()
    assert a % 16 == 0 and _JOBS.data_ptr() % 8 == 0
    vp1 = ctypes.c_void_p * 1
    per = l.rqhip_bf16_images_job_bytes(1)
    assert per > 0 and l.rqhip_bf16_images_job_bytes(70) == 70 * per
    assert l.rqhip_bf16_images_job_bytes(0) == 0 and l.rqhip_bf16_images_job_bytes(-3) == 0
    # tiles: one per 32 x 32, the jobs in order
    assert _fill(l) == (0, 2)
    assert _fill(l, rows=(32, 96, 384), cols=(32, 64, 1024), img_t=(ctypes.c_void_p * 3)(a, None, a)) == (0, 1 + 6 + 384)
    assert _fill(l, rows=(), cols=(), n=0) == (0, 0)
    # sizes: multiples of 32 only, -2
    for rows, cols in (((48,), (64,)), ((32,), (40,)), ((0,), (32,)), ((32,), (-32,)), ((16,), (32,))):
        rc, _ = _fill(l, rows=rows, cols=cols)
        assert rc == -2 and b"multiples of 32" in l.rqhip_last_error() and b"bf16_images" in l.rqhip_last_error()
    # null pointers
    assert _fill(l, n=-1)[0] == -1 and b"bad size" in l.rqhip_last_error()
    assert _fill(l, tiles=False)[0] == -1 and b"null pointer" in l.rqhip_last_error()
    assert l.rqhip_bf16_images_fill_jobs(None, vp1(a), vp1(a), None, (ctypes.c_int64 * 1)(32), (ctypes.c_int64 * 1)(32), 1,
                                         ctypes.byref(ctypes.c_int64())) == -1
    assert b"null pointer" in l.rqhip_last_error()
    for kw in ({"src": vp1(None)}, {"img": vp1(None)}):
        assert _fill(l, **kw)[0] == -1 and b"null pointer" in l.rqhip_last_error()
    # misaligned pointers: 16 bytes for the matrices and the images
    for kw in ({"src": vp1(a + 4)}, {"img": vp1(a + 8)}, {"img_t": vp1(a + 2)}):
        assert _fill(l, **kw)[0] == -1 and b"16-byte aligned" in l.rqhip_last_error()
    assert _fill(l, host=_JOBS.data_ptr() + 4)[0] == -1 and b"8-byte aligned" in l.rqhip_last_error()


def test_image_launch_checks_without_gpu():
    from rqhip import _lib
    l = _lib.lib()
    a = _HOST.data_ptr()
    assert l.rqhip_bf16_images(None, 0, 0, None) == 0          # no jobs: nothing to do, whatever the table
    assert l.rqhip_bf16_images(a, 0, 5, None) == 0
    assert l.rqhip_bf16_images(a, -1, 1, None) == -1 and b"bad size" in l.rqhip_last_error()
    assert l.rqhip_bf16_images(None, 2, 2, None) == -1 and b"null pointer" in l.rqhip_last_error()
    assert l.rqhip_bf16_images(a + 8, 2, 2, None) == -1 and b"16-byte aligned" in l.rqhip_last_error()
    for tiles in (0, 1, -4, 2 ** 31):                          # fewer tiles than jobs, or more than a grid
        assert l.rqhip_bf16_images(a, 2, tiles, None) == -1 and b"n_tiles" in l.rqhip_last_error()


def _ffn_fwd(l, *, N=8, d=64, F=96, p=0.0):
    return l.rqhip_t5_ffn_fwd_bf16w(None, None, None, N, d, F, p, None, None, None, None)


def _ffn_bwd(l, *, N=8, d=64, F=96, p=0.0):
    return l.rqhip_t5_ffn_bwd_bf16w(None, None, None, None, None, N, d, F, p, None, _HOST.data_ptr(), None, None, None, None)


@pytest.mark.parametrize("call,name", [(_ffn_fwd, b"t5_ffn_fwd_bf16w"), (_ffn_bwd, b"t5_ffn_bwd_bf16w")])
def test_ffn_argument_checks_without_gpu(call, name):
    from rqhip import _lib
    l = _lib.lib()
    for kw in ({"N": -1}, {"d": 0}, {"F": 0}):
        assert call(l, **kw) == -1 and b"bad sizes" in l.rqhip_last_error() and name in l.rqhip_last_error()
    for kw in ({"d": 48}, {"F": 48}, {"d": 16}, {"d": 544}, {"F": 8224}):
        assert call(l, **kw) == -2 and b"multiples of 32" in l.rqhip_last_error() and name in l.rqhip_last_error()
    for p in (1.0, -0.1, float("nan")):
        assert call(l, p=p) == -1 and b"0 <= p < 1" in l.rqhip_last_error() and name in l.rqhip_last_error()
    assert call(l) == -1 and b"null pointer" in l.rqhip_last_error() and name in l.rqhip_last_error()
    assert call(l, N=0) == 0 and call(l, N=0, d=48) == -2


def test_ffn_pointer_checks_without_gpu():
    from rqhip import _lib
    l = _lib.lib()
    N, d, F = 8, 64, 96
    a = _HOST.data_ptr()
    assert l.rqhip_t5_ffn_bwd_bf16w(a, a, a, a, a, N, d, F, 0.5, None, None, None, None, None, None) == 0   # nothing wanted
    assert l.rqhip_t5_ffn_fwd_bf16w(a, a, a, N, d, F, 0.1, None, a, a, None) == -1
    assert b"seed" in l.rqhip_last_error() and b"t5_ffn_fwd_bf16w" in l.rqhip_last_error()
    assert l.rqhip_t5_ffn_bwd_bf16w(a, a, a, a, a, N, d, F, 0.1, None, a, None, None, None, None) == -1
    assert b"seed" in l.rqhip_last_error() and b"t5_ffn_bwd_bf16w" in l.rqhip_last_error()
    assert l.rqhip_t5_ffn_bwd_bf16w(a, a, a, a, a, N, d, F, 0.0, None, None, a, None, None, None) == -3
    assert b"workspace" in l.rqhip_last_error() and b"t5_ffn_bwd_bf16w" in l.rqhip_last_error()
    for k in (1, 2):                                            # a misaligned image
        args = [a, a, a]
        args[k] = a + 8
        assert l.rqhip_t5_ffn_fwd_bf16w(*args, N, d, F, 0.0, None, a, a, None) == -1
        assert b"16-byte aligned" in l.rqhip_last_error()
        args = [a, a, a, a, a]
        args[k] = a + 8
        assert l.rqhip_t5_ffn_bwd_bf16w(*args, N, d, F, 0.0, None, a, a, a, a, None) == -1
        assert b"16-byte aligned" in l.rqhip_last_error()
    for k in range(5):
        args = [a, a, a, a, a]
        args[k] = None
        assert l.rqhip_t5_ffn_bwd_bf16w(*args, N, d, F, 0.0, None, a, a, a, a, None) == -1
        assert b"null pointer" in l.rqhip_last_error()
    for k in range(3):
        args = [a, a, a]
        args[k] = None
        assert l.rqhip_t5_ffn_fwd_bf16w(*args, N, d, F, 0.0, None, a, a, None) == -1
        assert b"null pointer" in l.rqhip_last_error()


def test_proj_argument_checks_without_gpu():
    from rqhip import _lib
    l = _lib.lib()
    a = _HOST.data_ptr()
    ptrs = (ctypes.c_void_p * 2)(a, a)
    lds = (ctypes.c_int64 * 2)(64, 64)

    def fwd(*, x=a, w=ptrs, y=ptrs, ld_y=lds, n=2, N=8, d_in=32, d_out=64, ld_x=32):
        return l.rqhip_t5_proj_fwd_bf16w(x, ld_x, w, y, ld_y, n, N, d_in, d_out, None)

    def bwd(*, x=a, w=ptrs, d_y=ptrs, ld_dy=lds, n=2, N=8, d_in=32, d_out=64, ld_x=32, d_x=a):
        return l.rqhip_t5_proj_bwd_bf16w(x, ld_x, w, d_y, ld_dy, n, N, d_in, d_out, d_x, None, None)

    for call, name in ((fwd, b"t5_proj_fwd_bf16w"), (bwd, b"t5_proj_bwd_bf16w")):
        assert call(N=-1) == -1 and b"bad sizes" in l.rqhip_last_error() and name in l.rqhip_last_error()
        for kw in ({"d_in": 48}, {"d_out": 16}, {"d_in": 544}, {"n": 9}, {"n": 0}):
            assert call(**kw) == -2 and b"multiples of 32" in l.rqhip_last_error() and name in l.rqhip_last_error()
        assert call(x=None) == -1 and b"null pointer" in l.rqhip_last_error() and name in l.rqhip_last_error()
        assert call(w=None) == -1 and b"null pointer" in l.rqhip_last_error()
        assert call(w=(ctypes.c_void_p * 2)(a, None)) == -1 and b"null pointer" in l.rqhip_last_error()
        assert call(w=(ctypes.c_void_p * 2)(a, a + 8)) == -1 and b"16-byte aligned" in l.rqhip_last_error()
        assert call(ld_x=30) == -1 and b"ld_x" in l.rqhip_last_error()
        assert call(x=a + 4) == -1 and b"16-byte aligned" in l.rqhip_last_error()
        assert call(N=0) == 0
    assert fwd(y=None) == -1 and b"null pointer" in l.rqhip_last_error()
    assert fwd(ld_y=(ctypes.c_int64 * 2)(64, 32)) == -1 and b"ld_y[1]" in l.rqhip_last_error()
    assert bwd(ld_dy=(ctypes.c_int64 * 2)(64, 66)) == -1 and b"ld_dy[1]" in l.rqhip_last_error()


def test_ops_reject_images_with_the_fp32_arithmetic():
    from rqhip import ops
    from rqhip._lib import RqHipError
    assert ops.T5_ARITHS == ("fp32", "bf16")
    x, wi, wo = torch.zeros(3, 32), torch.zeros(64, 32), torch.zeros(32, 64)
    i16, o16 = wi.bfloat16(), wo.bfloat16()
    calls = (lambda **kw: ops.t5_ffn_fwd(x, wi, wo, w_images=(i16, o16), **kw),
             lambda **kw: ops.t5_ffn_bwd(x, wi, wo, torch.zeros(3, 64), x, w_images=(o16, i16), **kw),
             lambda **kw: ops.t5_proj_fwd(x, [wi], w_images=[i16], **kw),
             lambda **kw: ops.t5_proj_bwd(x, [wi], [torch.zeros(3, 64)], w_images=[o16], **kw))
    for call in calls:
        with pytest.raises(RqHipError, match='w_images belong to arith="bf16"'):
            call()                                   # the default arithmetic is "fp32"
        with pytest.raises(RqHipError, match='w_images belong to arith="bf16"'):
            call(arith="fp32")
        with pytest.raises(RqHipError, match="arith must be one of"):
            call(arith="fp16")
        with pytest.raises(RqHipError, match="no CPU fallback"):
            call(arith="bf16")                       # the next check: these are host tensors
    for fn in (ops.t5_ffn_fwd, ops.t5_ffn_bwd, ops.t5_proj_fwd, ops.t5_proj_bwd):
        params = inspect.signature(fn).parameters
        assert params["w_images"].default is None and params["arith"].default == "fp32"
    for fn in (ops.bf16_images_alloc, lambda w: ops.bf16_images_jobs(w, [i16])):
        with pytest.raises(RqHipError, match="no CPU fallback"):
            fn([wi])


def test_weight_images_is_validated_by_model_and_stack():
    from modules.t5 import WEIGHT_IMAGES, T5Config, T5Stack, T5WeightImages
    assert WEIGHT_IMAGES == ("none", "bf16")
    keys = sorted(tiny_model(32, 32).state_dict())
    m = tiny_model(32, 32).eval()
    assert m.weight_images == "none" and m.encoder.encoder.weight_images == "none" and m.t5_decoder.weight_images == "none"
    with torch.no_grad():
        want = m(tiny_batch()).loss
        m.matmul_arith, m.ffn_impl, m.proj_impl, m.weight_images = "bf16", "hip", "hip", "bf16"
        got = m(tiny_batch()).loss          # host tensors: the operators, on which the attribute has no effect
    assert m.encoder.encoder.weight_images == "bf16" and m.t5_decoder.weight_images == "bf16"
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and sorted(m.state_dict()) == keys
    for stack in (m.encoder.encoder, m.t5_decoder):
        assert isinstance(stack.images, T5WeightImages) and stack.images.refreshes == 0 and stack.images.key is None
        assert not any("images" in n for n, _ in stack.named_buffers()) and "images" not in stack._modules
    m.weight_images = "fp8"
    with pytest.raises(ValueError, match="weight_images"):
        m(tiny_batch())
    stack = T5Stack(T5Config(16, d_model=32, num_heads=2, d_ff=64, num_layers=1)).eval()
    assert stack.weight_images == "none" and stack.weight_images_mode() == "none"
    x = torch.randn(2, 3, 32)
    want = stack(x)
    stack.weight_images, stack.matmul_arith = "bf16", "bf16"
    assert stack.matmul_plan(x) == (None, None, None) and torch.equal(stack(x), want)
    stack.weight_images = "bogus"
    with pytest.raises(ValueError, match="weight_images"):
        stack(x)
    stack.matmul_arith = "fp32"             # validated on every path, like matmul_arith
    with pytest.raises(ValueError, match="weight_images"):
        stack(x)


def test_train_has_no_parameter_for_the_images():
    import train_decoder
    assert "weight_images" not in inspect.signature(train_decoder.train).parameters
    assert "weight_images" in train_decoder.__doc__


def test_the_holders_key_sees_every_way_a_weight_changes():
    from modules.t5 import T5Config, T5Stack, T5WeightImages
    from rqhip import optim
    cfg = T5Config(16, d_model=32, num_heads=2, d_ff=64, num_layers=2, is_decoder=True)
    stack = T5Stack(cfg).eval()
    weights = stack.image_weights(True, True)
    # two blocks: self- and cross-attention q, k, v, o and the feed-forward's wi, wo
    assert len(weights) == 2 * (4 + 4 + 2) and len({id(w) for w in weights}) == len(weights)
    assert len(stack.image_weights(True, False)) == 4 and len(stack.image_weights(False, True)) == 16
    key = T5WeightImages.key_of(weights)
    assert key[-1] == optim.generation() and len(key) == len(weights) + 1
    enc = torch.randn(2, 5, 32)
    with torch.no_grad():
        stack(torch.randn(2, 3, 32), encoder_hidden_states=enc)
    assert T5WeightImages.key_of(stack.image_weights(True, True)) == key        # a forward changes nothing
    seen = {key}

    def changed():
        k = T5WeightImages.key_of(stack.image_weights(True, True))
        new = k not in seen
        seen.add(k)
        return new

    with torch.no_grad():
        stack.block[1].layer[-1].DenseReluDense.wo.weight.add_(1.0)             # an in-place operator
    assert changed()
    stack.load_state_dict({k: v.clone() for k, v in stack.state_dict().items()})
    assert changed()
    p = stack.block[0].layer[1].EncDecAttention.k.weight
    p.data = p.data.clone()                                                      # a .data swap
    assert changed()
    opt = torch.optim.AdamW(stack.parameters(), lr=1e-3)
    stack(torch.randn(2, 3, 32), encoder_hidden_states=enc).sum().backward()
    opt.step()
    assert changed()
    before = optim.generation()
    flat = optim.FlatAdamW(stack.parameters(), lr=1e-3)
    with pytest.raises(Exception):                                               # host tensors: it refuses, and still counts
        flat.step()
    assert optim.generation() == before + 1 and changed()
    # the holder compares exactly this key
    holder = T5WeightImages()
    assert holder.key is None and not holder.current(weights)
    holder.key = T5WeightImages.key_of(weights)
    assert holder.current(weights)
    with torch.no_grad():
        weights[0].mul_(2.0)
    assert not holder.current(weights)
    holder.invalidate()
    assert holder.key is None and holder.arena is None and holder.jobs is None
