"""bf16 saved activations on the host: the size queries, the new entry points' argument checks (every one before any HIP
call, with a host buffer standing in for device memory as in tests/test_t5_weight_images_host.py), the index formula of
the blocked activation image restated in NumPy against ops.t5_act_image_rows, the `saved` keyword of the ops and
`saved_activations` on the stack and on the model.  No GPU needed."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from retrieval_cases import tiny_batch, tiny_model

ENTRIES = ("rqhip_t5_ffn_fwd_bf16a", "rqhip_t5_ffn_bwd_bf16a", "rqhip_t5_ffn_fwd_bf16wa", "rqhip_t5_ffn_bwd_bf16wa")
QUERIES = ("rqhip_t5_ffn_act_image_bytes", "rqhip_t5_ffn_bwd_bf16a_workspace_bytes")
_HOST = torch.zeros(8 * 96 + 64)


def test_symbols_are_exported_declared_and_bound():
    from rqhip import _lib
    handle = ctypes.CDLL(_lib.SO_PATH)
    text = open(os.path.join(ROOT, "include", "rqhip.h")).read()
    declared = set(re.findall(r"\b(rqhip_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    for name in ENTRIES + QUERIES:
        assert hasattr(handle, name) and name in declared and name in _lib.SIGNATURES, name
    for who in ("fwd", "bwd"):      # the weight-image variant has the parameter list of the plain one
        assert _lib.SIGNATURES[f"rqhip_t5_ffn_{who}_bf16wa"] == _lib.SIGNATURES[f"rqhip_t5_ffn_{who}_bf16a"]
    assert _lib.lib().rqhip_version() == 462
    # the contract names the layout and the one difference from the bf16 arm
    assert "((b * C + c) * 32 + 8 * kq + ks)" in text and "h * s <= 2^-134" in text


def test_size_queries():
    from rqhip import _lib, ops
    l = _lib.lib()
    image = l.rqhip_t5_ffn_act_image_bytes
    for N, C in ((1, 32), (16, 32), (32, 64), (33, 512), (40, 1024), (16385, 32), (327680, 1024)):
        assert image(N, C) == 2 * 32 * ((N + 31) // 32) * C, (N, C)
        assert ops.t5_act_image_numel(N, C) * 2 == image(N, C)
    assert image(0, 32) == 0 and image(-1, 32) == 0
    for C in (0, 16, 48, -32):
        assert image(8, C) == 0, C
    work = l.rqhip_t5_ffn_bwd_bf16a_workspace_bytes
    for N, d, F in ((1, 32, 32), (17, 96, 160), (40, 384, 1024), (16385, 32, 32)):
        assert work(N, d, F) == image(N, d) + image(N, F) == 64 * ((N + 31) // 32) * (d + F)
    assert work(0, 32, 32) == 0 and work(-1, 32, 32) == 0
    assert work(8, 48, 32) == 0 and work(8, 32, 8224) == 0 and work(8, 544, 32) == 0       # unsupported shapes
    # half of the fp32 arm's bytes wherever N is a multiple of 32: g [N, F] fp32 alone is 4 N F
    assert work(64, 384, 1024) == (4 * 64 * (384 + 1024)) // 2


def _fwd(l, name, *, N=8, d=64, F=96, p=0.0):
    return getattr(l, name)(None, None, None, N, d, F, p, None, None, None, None, None)


def _bwd(l, name, *, N=8, d=64, F=96, p=0.0):
    return getattr(l, name)(None, None, None, None, None, N, d, F, p, _HOST.data_ptr(), None, None, None, None)


@pytest.mark.parametrize("name", ENTRIES)
def test_argument_checks_without_gpu(name):
    from rqhip import _lib
    l = _lib.lib()
    call = _fwd if "_fwd_" in name else _bwd
    tag = name[len("rqhip_"):].encode()
    for kw in ({"N": -1}, {"d": 0}, {"F": 0}):
        assert call(l, name, **kw) == -1 and b"bad sizes" in l.rqhip_last_error() and tag in l.rqhip_last_error()
    for kw in ({"d": 48}, {"F": 48}, {"d": 16}, {"d": 544}, {"F": 8224}):
        assert call(l, name, **kw) == -2 and b"multiples of 32" in l.rqhip_last_error() and tag in l.rqhip_last_error()
    for p in (1.0, -0.1, float("nan")):
        assert call(l, name, p=p) == -1 and b"0 <= p < 1" in l.rqhip_last_error() and tag in l.rqhip_last_error()
    assert call(l, name) == -1 and b"null pointer" in l.rqhip_last_error() and tag in l.rqhip_last_error()
    assert call(l, name, N=0) == 0 and call(l, name, N=0, d=48) == -2


@pytest.mark.parametrize("suffix", ["a", "wa"])
def test_pointer_and_workspace_checks_without_gpu(suffix):
    from rqhip import _lib
    l = _lib.lib()
    fwd, bwd = getattr(l, "rqhip_t5_ffn_fwd_bf16" + suffix), getattr(l, "rqhip_t5_ffn_bwd_bf16" + suffix)
    N, d, F = 8, 64, 96
    a = _HOST.data_ptr()
    assert a % 16 == 0
    assert bwd(a, a, a, a, a, N, d, F, 0.5, None, None, None, None, None) == 0           # nothing wanted; no seed exists
    assert fwd(a, a, a, N, d, F, 0.1, None, a, a, a, None) == -1 and b"seed" in l.rqhip_last_error()
    # a weight gradient without the workspace: d_wi, and d_wo alone, which needs it for dy16
    for wanted in ((a, None), (None, a), (a, a)):
        assert bwd(a, a, a, a, a, N, d, F, 0.0, None, *wanted, None, None) == -3
        assert b"workspace" in l.rqhip_last_error() and b"bf16a_workspace_bytes" in l.rqhip_last_error()
    for k in range(5):                                            # x16, wi, wo, hd16, d_y
        args = [a] * 5
        args[k] = None
        assert bwd(*args, N, d, F, 0.0, a, a, a, a, None) == -1 and b"null pointer" in l.rqhip_last_error()
        args[k] = a + 8
        assert bwd(*args, N, d, F, 0.0, a, a, a, a, None) == -1 and b"16-byte aligned" in l.rqhip_last_error()
    assert bwd(a, a, a, a, a, N, d, F, 0.0, a, a, a, a + 8, None) == -1 and b"16-byte aligned" in l.rqhip_last_error()
    for k in range(3):                                            # x, wi, wo
        args = [a] * 3
        args[k] = None
        assert fwd(*args, N, d, F, 0.0, None, a, a, a, None) == -1 and b"null pointer" in l.rqhip_last_error()
    assert fwd(a, a, a, N, d, F, 0.0, None, None, a, a, None) == -1 and b"null pointer" in l.rqhip_last_error()   # y
    for images in ((a + 8, a), (a, a + 8)):                       # a misaligned hd16 or x16
        assert fwd(a, a, a, N, d, F, 0.0, None, a, *images, None) == -1 and b"16-byte aligned" in l.rqhip_last_error()


def _image_index(n, c, C):
    """Section 'blocked image' of include/rqhip.h, as written there."""
    b, rho = n >> 5, n & 31
    kq, ks = rho & 3, rho >> 2
    return (b * C + c) * 32 + 8 * kq + ks


@pytest.mark.parametrize("N", [1, 16, 33])
@pytest.mark.parametrize("C", [32, 96])
def test_act_image_rows_is_the_index_formula(N, C):
    from rqhip import ops
    nb = (N + 31) // 32
    # a distinct finite bf16 pattern per buffer element (fewer than 30000 elements; 30000 < 0x7F80)
    buf = np.arange(nb * C * 32, dtype=np.int64)
    img = torch.from_numpy((buf % 30000).astype(np.int16)).view(torch.bfloat16)
    want = np.empty((N, C), dtype=np.int16)
    for n in range(N):
        for c in range(C):
            want[n, c] = buf[_image_index(n, c, C)] % 30000
    got = ops.t5_act_image_rows(img, N, C)
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (N, C) and got.is_contiguous()
    assert np.array_equal(got.view(torch.int16).numpy(), want)
    # the lane's fragment: rows 4 ks + kq of block b, column c, are 8 consecutive elements from a 16-byte boundary
    for kq in range(4):
        first = _image_index(kq, 5, C)
        assert first % 8 == 0 and [_image_index(4 * ks + kq, 5, C) for ks in range(8)] == list(range(first, first + 8))


def test_act_image_rows_checks_its_argument():
    from rqhip import ops
    from rqhip._lib import RqHipError
    with pytest.raises(RqHipError, match="t5_act_image_rows"):
        ops.t5_act_image_rows(torch.zeros(32 * 32, dtype=torch.bfloat16), 33, 32)        # two blocks are 2048 elements
    with pytest.raises(RqHipError, match="t5_act_image_rows"):
        ops.t5_act_image_rows(torch.zeros(32 * 32), 1, 32)                               # not bfloat16
    with pytest.raises(RqHipError, match="t5_act_image_rows"):
        ops.t5_act_image_rows(torch.zeros(32 * 48, dtype=torch.bfloat16), 1, 48)         # C no multiple of 32


def test_ops_take_saved_with_the_bf16_arithmetic_only():
    from rqhip import ops
    from rqhip._lib import RqHipError
    assert ops.T5_SAVED == ("fp32", "bf16")
    x, wi, wo = torch.zeros(3, 32), torch.zeros(64, 32), torch.zeros(32, 64)
    pair = (torch.zeros(32 * 64, dtype=torch.bfloat16), torch.zeros(32 * 32, dtype=torch.bfloat16))
    calls = (lambda **kw: ops.t5_ffn_fwd(x, wi, wo, saved="bf16", **kw),
             lambda **kw: ops.t5_ffn_bwd(None, wi, wo, pair, x, saved="bf16", **kw))
    for call in calls:
        with pytest.raises(RqHipError, match='saved="bf16" belongs to arith="bf16"'):
            call()                                   # the default arithmetic is "fp32"
        with pytest.raises(RqHipError, match='saved="bf16" belongs to arith="bf16"'):
            call(arith="fp32")
        with pytest.raises(RqHipError, match="arith must be one of"):
            call(arith="fp16")
        with pytest.raises(RqHipError, match="no CPU fallback"):
            call(arith="bf16")                       # the next check: these are host tensors
    with pytest.raises(RqHipError, match="saved must be one of"):
        ops.t5_ffn_fwd(x, wi, wo, arith="bf16", saved="fp16")
    with pytest.raises(RqHipError, match="pair"):
        ops.t5_ffn_bwd(None, wi, wo, torch.zeros(3, 64), x, arith="bf16", saved="bf16")
    for fn in (ops.t5_ffn_fwd, ops.t5_ffn_bwd):
        assert inspect.signature(fn).parameters["saved"].default == "fp32"


def test_saved_activations_is_validated_by_model_and_stack():
    from modules.t5 import SAVED_ACTIVATIONS, T5Config, T5Stack
    assert SAVED_ACTIVATIONS == ("fp32", "bf16")
    m = tiny_model(32, 32).eval()
    keys = sorted(m.state_dict())
    assert m.saved_activations == "fp32"
    assert m.encoder.encoder.saved_activations == "fp32" and m.t5_decoder.saved_activations == "fp32"
    with torch.no_grad():
        want = m(tiny_batch()).loss
    m.matmul_arith, m.ffn_impl, m.saved_activations = "bf16", "hip", "bf16"
    got = m(tiny_batch()).loss          # host tensors, under grad: the operators, on which the attribute has no effect
    assert m.encoder.encoder.saved_activations == "bf16" and m.t5_decoder.saved_activations == "bf16"
    assert torch.equal(got.detach().view(torch.int32), want.view(torch.int32)) and sorted(m.state_dict()) == keys
    m.saved_activations = "fp16"
    with pytest.raises(ValueError, match="saved_activations"):
        m(tiny_batch())
    stack = T5Stack(T5Config(16, d_model=32, num_heads=2, d_ff=64, num_layers=1)).eval()
    assert stack.saved_activations == "fp32" and stack.saved_activations_mode() == "fp32"
    x = torch.randn(2, 3, 32)
    want = stack(x)
    stack.saved_activations, stack.matmul_arith = "bf16", "bf16"
    assert torch.equal(stack(x), want)
    stack.saved_activations = "bogus"
    with pytest.raises(ValueError, match="saved_activations"):
        stack(x)
    stack.matmul_arith = "fp32"             # validated on every path, like weight_images
    with pytest.raises(ValueError, match="saved_activations"):
        stack(x)


def test_train_has_no_parameter_for_it():
    import train_decoder
    assert "saved_activations" not in inspect.signature(train_decoder.train).parameters
