"""The fused semantic-id input embedding (csrc/sid_embed.hip, rqhip_sid_embed_fwd / _bwd; embed_impl = "hip") on the
host: the supported shapes, the argument checks of the C entry points, which all come before any HIP call, the wrappers'
own checks, the option on the model and the fall-back to the operators on host tensors.  No GPU needed."""
import pytest
import torch

from retrieval_cases import tiny_batch, tiny_model


def _fwd(l, *, B=3, items=2, L=3, ld_item=4, K=16, d=64, mask=None, elt=1, prefix=None, prefix_rows=0, data=None):
    # the data pointers stay null unless `data` is given: they are checked last
    return l.rqhip_sid_embed_fwd(data, mask, elt, B, items, L, ld_item, K, d, data, None, prefix, None, 0, prefix_rows,
                                 data, None, None)


def _bwd(l, *, B=3, items=2, L=3, ld_item=4, K=16, d=64, mask=None, elt=1, prefix=None, prefix_rows=0, data=None):
    return l.rqhip_sid_embed_bwd(data, data, mask, elt, B, items, L, ld_item, K, d, 0, int(prefix is not None), None, 0,
                                 prefix_rows, data, None, None, None, 0, None)


def test_supported_shapes():
    from rqhip import _lib, ops
    l = _lib.lib()
    for d, want in ((4, True), (1024, True), (128, True), (0, False), (6, False), (1028, False), (-4, False)):
        assert bool(l.rqhip_sid_embed_supported(d, 3)) == want, d
    for L, want in ((0, False), (1, True), (8, True), (9, False), (-1, False)):
        assert bool(l.rqhip_sid_embed_supported(64, L)) == want, L
    assert ops.sid_embed_supported(torch.float32, 128, 3)
    for dtype in (torch.float16, torch.bfloat16, torch.float64):
        assert not ops.sid_embed_supported(dtype, 128, 3)
    # sized by the shape alone, the same on every call
    for shape in ((64, 20, 3, 256, 128), (0, 1, 1, 1, 4), (9, 64, 2, 1, 1024)):
        assert l.rqhip_sid_embed_bwd_workspace_bytes(*shape) == l.rqhip_sid_embed_bwd_workspace_bytes(*shape)


@pytest.mark.parametrize("call,name", [(_fwd, b"sid_embed_fwd"), (_bwd, b"sid_embed_bwd")])
def test_argument_checks_without_gpu(call, name):
    """Host buffers stand in for device memory: every call below is refused before it could be dereferenced."""
    from rqhip import _lib
    l = _lib.lib()
    a = torch.zeros(64).data_ptr()
    err = l.rqhip_last_error
    assert call(l, B=-1) == -1 and b"bad sizes" in err() and name in err()
    assert call(l, items=0) == -1 and b"bad sizes" in err()
    assert call(l, K=0) == -1 and b"bad sizes" in err()
    assert call(l, ld_item=2) == -1 and b"ld_item >= L" in err() and name in err()
    for d in (0, 6, 1028):
        assert call(l, d=d) == -1 and b"multiple of 4" in err() and name in err()
    for L in (0, 9):
        assert call(l, L=L, ld_item=9) == -1 and b"L in 1 .. 8" in err()
    for elt in (0, 2, 4, 16):
        assert call(l, mask=a, elt=elt) == -1 and b"mask element size" in err() and name in err()
    assert call(l, prefix=a, prefix_rows=0) == -1 and b"prefix_rows" in err() and name in err()
    # fully valid sizes, null data: refused last, and by name
    assert call(l) == -1 and b"null pointer" in err() and name in err()
    assert call(l, mask=a, elt=8, prefix=a, prefix_rows=7) == -1 and b"null pointer" in err()
    # float4 accesses
    assert call(l, data=a + 4) == -1 and b"16-byte aligned" in err()
    # an empty batch: nothing to do, whatever the pointers
    assert call(l, B=0) == 0


def test_wrappers_check_dtypes_and_shapes():
    from rqhip import ops
    from rqhip._lib import RqHipError
    ids, table = torch.zeros(3, 8, dtype=torch.long), torch.zeros(48, 8)
    with pytest.raises(RqHipError, match="table must be float32"):
        ops.sid_embed_fwd(ids, None, table.double(), 3, 4)
    with pytest.raises(RqHipError, match="ids must be an int64"):
        ops.sid_embed_fwd(ids.float(), None, table, 3, 4)
    with pytest.raises(RqHipError, match="not items \\* ld_item"):
        ops.sid_embed_fwd(ids[:, :7], None, table, 3, 4)
    with pytest.raises(RqHipError, match="not items \\* ld_item"):
        ops.sid_embed_bwd(torch.zeros(3, 6, 8), ids[:, :7], None, 3, 4, 16, has_sep=False)
    with pytest.raises(RqHipError, match="mask must be a bool or int64"):
        ops.sid_embed_fwd(ids, torch.ones(3, 8), table, 3, 4)
    with pytest.raises(RqHipError, match="sep must hold"):
        ops.sid_embed_fwd(ids, None, table, 3, 4, sep=torch.zeros(4))
    with pytest.raises(RqHipError, match="d_x must be a float32"):
        ops.sid_embed_bwd(torch.zeros(3, 6, 8).double(), ids, None, 3, 4, 16, has_sep=False)
    with pytest.raises(RqHipError, match="not supported"):
        ops.sid_embed_fwd(ids, None, torch.zeros(48, 6), 3, 4)
    # well-formed host tensors: there is no CPU path
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.sid_embed_fwd(ids, None, table, 3, 4)
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.sid_embed_bwd(torch.zeros(3, 6, 8), ids, None, 3, 4, 16, has_sep=False)


def test_option_values_and_state_dict():
    from modules.model import EMBED_IMPLS
    assert EMBED_IMPLS == ("torch", "hip")
    batch = tiny_batch()
    keys = sorted(tiny_model().state_dict())
    m = tiny_model().eval()
    assert m.embed_impl == "torch" and not m.hip_embed_active(batch.sem_ids, batch.seq_mask)
    m.embed_impl = "hip"
    assert not m.hip_embed_active(batch.sem_ids, batch.seq_mask)       # host tensors
    assert sorted(m.state_dict()) == keys and [n for n, _ in m.named_modules()] == [n for n, _ in
                                                                                   tiny_model().named_modules()]
    m.embed_impl = "bogus"
    with pytest.raises(ValueError, match="embed_impl"):
        m.hip_embed_active(batch.sem_ids, batch.seq_mask)
    with pytest.raises(ValueError, match="embed_impl"):
        m(batch)


def test_hip_embed_on_host_tensors_is_the_operators():
    m = tiny_model().eval()
    batch = tiny_batch()

    def run():
        m.zero_grad(set_to_none=True)
        out = m(batch)
        out.loss.backward()
        return out.loss.detach(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}

    want, want_g = run()
    m.embed_impl = "hip"
    got, got_g = run()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and sorted(got_g) == sorted(want_g) and len(got_g) > 10
    for n in want_g:
        assert torch.equal(got_g[n], want_g[n]), n
