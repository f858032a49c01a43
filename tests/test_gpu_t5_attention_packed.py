"""The packed attention calls (ops.t5_attention_packed, _fwd_train, _bwd; csrc/t5_attention.hip) against today's padded
calls.

The packed kernels keep the padded call's index laws (bias by j - i, dropout element ((b * H + h) * Tq + i) * Tk + j, the
kernel instantiation and LDS layout of the bounds) and only shorten a workgroup's loops to its own lengths.  In the padded
call with the prefix key mask a masked key's weight is exactly 0, so is its dS, and a padded query row with d_out = 0
adds exact zeros to dk, dv and the bias partials.  Hence the gate is bits, not a tolerance: on every valid element of
out, lse, dq, dk and dv, on the whole of dtable, and between two runs.

Reference: ops.t5_attention_fwd_train / _bwd on the scattered (padded) tensors -- whose padded rows hold random finite
values, not zeros -- with key_mask = the prefix mask, d_out zero on padded query rows and the same seed.

Shapes: 4 groups, H in {1, 6}, bounds T in {17, 81, 256}: one, six and sixteen key tiles, the three instantiations.
Lengths: 1, the tile edges 15 / 16 / 17, the bound itself.  Forms: the encoder's (both tables, the bias table of
retrieval_cases._bias_module) and the cross-attention's (dense queries, Tq = 4, packed K/V, no bias).  p in {0, 0.1, 0.5}
with a seed that has bits above the low 32."""
import functools

import pytest
import torch

from retrieval_cases import _bias_module, same_bits

pytestmark = pytest.mark.gpu

B, TQ_CROSS = 4, 4
SEED = (5 << 40) + 12345
LENGTHS = {"mix": lambda T: [T, 1, 17, 16], "edges": lambda T: [15, 16, 17, 1]}


def _cu(lengths):
    cu = torch.zeros(len(lengths) + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(torch.tensor(lengths), 0)
    return cu.cuda()


def _valid(lengths, T):
    return (torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]).cuda()      # [B, T] prefix mask


@functools.lru_cache(maxsize=None)
def _tensors(T, H, which):
    """Padded q, k, v, d_out of the encoder form and of the cross form (random everywhere, padding included), the prefix
    mask, the table of cumulative lengths and the bias table."""
    lengths = LENGTHS[which](T)
    g = torch.Generator().manual_seed(100 * T + H)
    inner = H * 64
    mk = lambda *s: torch.randn(*s, generator=g).cuda()
    q, k, v, d_out = mk(B, T, inner) * 1.5, mk(B, T, inner), mk(B, T, inner), mk(B, T, inner)
    qc, d_outc = mk(B, TQ_CROSS, inner) * 1.5, mk(B, TQ_CROSS, inner)
    keep = _valid(lengths, T)
    att = _bias_module(H, False, 3)
    with torch.no_grad():
        table, offset = att.delta_table(T, T)
        table = table.clone()
    return dict(q=q, k=k, v=v, d_out=d_out * keep[:, :, None], qc=qc, d_outc=d_outc, keep=keep, cu=_cu(lengths),
                table=table, offset=offset, lengths=lengths)


def _seed(p):
    return torch.tensor([SEED], dtype=torch.int64, device="cuda") if p > 0 else None


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("which", list(LENGTHS))
@pytest.mark.parametrize("H", [1, 6])
@pytest.mark.parametrize("T", [17, 81, 256])
def test_encoder_form_has_the_padded_bits(T, H, which, p):
    from rqhip import ops
    t = _tensors(T, H, which)
    keep, cu, seed = t["keep"], t["cu"], _seed(p)
    kw = dict(bias_by_delta=t["table"], bias_offset=t["offset"], p=p, seed=seed)
    out_r, lse_r = ops.t5_attention_fwd_train(t["q"], t["k"], t["v"], H, key_mask=keep, **kw)
    dq_r, dk_r, dv_r, dtable_r = ops.t5_attention_bwd(t["q"], t["k"], t["v"], out_r, lse_r, t["d_out"], H, key_mask=keep,
                                                      **kw)
    pk = dict(cu_q=cu, cu_k=cu, max_q=T, max_k=T, **kw)
    q, k, v, d_out = (t[n][keep] for n in ("q", "k", "v", "d_out"))          # [N, inner]: the valid rows in order

    def run():
        out, lse = ops.t5_attention_packed_fwd_train(q, k, v, H, **pk)
        return (out, lse) + tuple(ops.t5_attention_packed_bwd(q, k, v, out, lse, d_out, H, **pk))

    out, lse, dq, dk, dv, dtable = got = run()
    N = sum(t["lengths"])
    assert out.shape == (N, H * 64) and lse.shape == (N, H) and dq.shape == dk.shape == dv.shape == out.shape
    assert same_bits(out, out_r[keep]), "out"
    assert same_bits(lse, lse_r.permute(0, 2, 1)[keep]), "lse"
    assert same_bits(dq, dq_r[keep]), "dq"
    assert same_bits(dk, dk_r[keep]), "dk"
    assert same_bits(dv, dv_r[keep]), "dv"
    assert same_bits(dtable, dtable_r), "dtable"
    assert bool(dtable.any()) and bool(dq.any())
    for x, y in zip(got, run()):
        assert same_bits(x, y), "two runs"
    if p == 0:
        assert same_bits(ops.t5_attention_packed(q, k, v, H, cu_q=cu, cu_k=cu, max_q=T, max_k=T,
                                                 bias_by_delta=t["table"], bias_offset=t["offset"]), out)


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("which", list(LENGTHS))
@pytest.mark.parametrize("H", [1, 6])
@pytest.mark.parametrize("T", [17, 81, 256])
def test_cross_form_has_the_padded_bits(T, H, which, p):
    from rqhip import ops
    t = _tensors(T, H, which)
    keep, cu, seed = t["keep"], t["cu"], _seed(p)
    q, d_out = t["qc"], t["d_outc"]
    out_r, lse_r = ops.t5_attention_fwd_train(q, t["k"], t["v"], H, key_mask=keep, p=p, seed=seed)
    dq_r, dk_r, dv_r, none_r = ops.t5_attention_bwd(q, t["k"], t["v"], out_r, lse_r, d_out, H, key_mask=keep, p=p,
                                                    seed=seed)
    k, v = t["k"][keep], t["v"][keep]
    pk = dict(cu_k=cu, max_k=T, p=p, seed=seed)

    def run():
        out, lse = ops.t5_attention_packed_fwd_train(q, k, v, H, **pk)
        return (out, lse) + tuple(ops.t5_attention_packed_bwd(q, k, v, out, lse, d_out, H, **pk))

    out, lse, dq, dk, dv, dtable = got = run()
    assert dtable is None and none_r is None
    assert out.shape == q.shape and lse.shape == (B, H, TQ_CROSS) and dk.shape == dv.shape == k.shape
    assert same_bits(out, out_r) and same_bits(lse, lse_r), "out, lse"
    assert same_bits(dq, dq_r), "dq"
    assert same_bits(dk, dk_r[keep]) and same_bits(dv, dv_r[keep]), "dk, dv"
    for x, y in zip(got[:5], run()[:5]):
        assert same_bits(x, y), "two runs"
    if p == 0:
        assert same_bits(ops.t5_attention_packed(q, k, v, H, cu_k=cu, max_k=T), out)


def test_dropout_decisions_are_the_padded_elements():
    """With v = 1 and one head-width of ones, out[i] = sum_j P_ij keep_ij / (1 - p): against the published decision of the
    padded index law, ops.t5_attention_dropout_keep(seed, B, H, T, T, p)."""
    from rqhip import ops
    T, H, p = 17, 1, 0.5
    lengths = [17, 1, 16, 15]
    cu, keep = _cu(lengths), _valid(lengths, T)
    N = sum(lengths)
    q = torch.zeros(N, 64, device="cuda")                                   # uniform weights 1 / len
    k = torch.randn(N, 64, generator=torch.Generator().manual_seed(0)).cuda()
    v = torch.ones(N, 64, device="cuda")
    seed = _seed(p)
    out, _ = ops.t5_attention_packed_fwd_train(q, k, v, H, cu_q=cu, cu_k=cu, max_q=T, max_k=T, p=p, seed=seed)
    drop = ops.t5_attention_dropout_keep(seed, B, H, T, T, p)[:, 0]          # [B, T, T]
    kept = (drop & keep[:, None, :]).sum(-1).float()                        # kept valid keys per (b, i)
    want = (kept / torch.tensor(lengths, device="cuda")[:, None] * 2.0)[keep]
    assert torch.allclose(out[:, 0], want, rtol=1e-6, atol=0)


def test_an_empty_group_is_empty():
    """A group without keys gives out = 0, lse = -inf and dq = 0, not 0 / 0; its neighbours are computed as ever."""
    from rqhip import ops
    T, H = 17, 1
    g = torch.Generator().manual_seed(4)
    k, v = torch.randn(20, 64, generator=g).cuda(), torch.randn(20, 64, generator=g).cuda()
    cu_k = _cu([17, 0, 3, 0])
    q, d_out = torch.randn(B, TQ_CROSS, 64, generator=g).cuda(), torch.randn(B, TQ_CROSS, 64, generator=g).cuda()
    out, lse = ops.t5_attention_packed_fwd_train(q, k, v, H, cu_k=cu_k, max_k=T)
    dq, dk, dv, _ = ops.t5_attention_packed_bwd(q, k, v, out, lse, d_out, H, cu_k=cu_k, max_k=T)
    for b in (1, 3):
        assert not bool(out[b].any()) and bool(torch.isneginf(lse[b]).all()) and not bool(dq[b].any())
    for x in (out, dq, dk, dv):
        assert bool(torch.isfinite(x).all())
    assert bool(out[0].any()) and bool(dq[2].any()) and bool(dk.any(dim=1).all()) and bool(dv.any(dim=1).all())


def test_malformed_host_arguments_raise():
    from rqhip import ops
    from rqhip._lib import RqHipError
    T, H = 17, 1
    t = _tensors(T, H, "mix")
    keep, cu = t["keep"], t["cu"]
    q, k, v = (t[n][keep] for n in ("q", "k", "v"))
    ok = dict(cu_q=cu, cu_k=cu, max_q=T, max_k=T)
    ops.t5_attention_packed(q, k, v, H, **ok)
    assert ops.t5_attention_packed_supported(torch.float32, 64, H, T, T)
    assert not ops.t5_attention_packed_supported(torch.float32, 64, H, 257, 257)
    for fn in (ops.t5_attention_packed, ops.t5_attention_packed_fwd_train):
        with pytest.raises(RqHipError):
            fn(q, k, v, H, causal=True, **ok)
        with pytest.raises(RqHipError):
            fn(q, k, v, H, key_mask=keep, **ok)
        with pytest.raises(RqHipError):
            fn(q, k, v, H, **{**ok, "cu_k": cu.long()})                      # the table's dtype
        with pytest.raises(RqHipError):
            fn(q, k, v, H, **{**ok, "cu_k": cu[:-1]})                        # the table's length
        with pytest.raises(RqHipError):
            fn(q, k, v, H, max_q=T, max_k=T)                                 # no table at all
        with pytest.raises(RqHipError):
            fn(q, k, v, H, cu_q=cu, cu_k=cu)                                 # no bounds
        with pytest.raises(RqHipError):
            fn(q, k, v, H, **{**ok, "max_k": 257})                           # beyond the short kernel
        with pytest.raises(RqHipError):
            fn(t["qc"], k, v, H, cu_k=cu[:-1], max_k=T)                      # dense q of 4 groups, a table of 3
    out, lse = ops.t5_attention_packed_fwd_train(q, k, v, H, **ok)
    with pytest.raises(RqHipError):
        ops.t5_attention_packed_bwd(q, k, v, out, lse, out, H, causal=True, **ok)
    with pytest.raises(RqHipError):
        ops.t5_attention_packed_bwd(q, k, v, out, lse.t().contiguous(), out, H, **ok)   # lse is [N, H]
    # the C entry points say the same without the wrapper's help (and without touching the device)
    from rqhip import _lib
    l = _lib.lib()
    rc = l.rqhip_t5_attention_packed(q.data_ptr(), 64, k.data_ptr(), v.data_ptr(), 64, B, q.shape[0], k.shape[0], H, 64, T,
                                     T, cu.data_ptr(), cu.data_ptr(), None, 0, 0, None, 1, q.data_ptr(), 64, None)
    assert rc == _lib.EARG and b"causal" in l.rqhip_last_error()
    rc = l.rqhip_t5_attention_packed(q.data_ptr(), 64, k.data_ptr(), v.data_ptr(), 64, B, q.shape[0], k.shape[0], H, 64, T,
                                     T, None, None, None, 0, 0, None, 0, q.data_ptr(), 64, None)
    assert rc == _lib.EARG and b"table" in l.rqhip_last_error()
