"""ops.t5_attention_packed_beams (csrc/t5_attention.hip: rqhip_t5_attention_packed_beams), the cross-attention of a
cached decode step over packed encoder rows: R = groups * beams dense query rows, rows b * beams .. reading the packed
K/V group b.

The call runs the packed kernel body with the dense arm's query rows, so the gate is bits, not a tolerance: on every
query it is torch.equal to ops.t5_attention on the K/V scattered into [groups, bound, H * 64] with the prefix key mask
(a masked key's weight is exactly 0; the padding slots hold finite random values, since 0 * NaN is not 0), and at
beams = 1 also to ops.t5_attention_packed(cu_q=None).  One case goes through retrieval_cases.attention_gate against the
operators in fp64, so that the gate does not rest on the padded kernel alone.

Shapes: H = 2, four groups with 17, 1, 16 and 5 keys under the bound 17 (a group that crosses the 16-key tile edge, a
single key, an exact tile); beams 1, 3, 10 and 17 (17: a second query tile with one live row); Tq 1 and 2; the bound 256
with lengths 256 and 1 for the largest instantiation."""
import functools

import pytest
import torch

from retrieval_cases import attention_gate

pytestmark = pytest.mark.gpu

H, INNER = 2, 128
LENGTHS, BOUND = [17, 1, 16, 5], 17


def _cu(lengths):
    cu = torch.zeros(len(lengths) + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(torch.tensor(lengths), 0)
    return cu.cuda()


def _valid(lengths, T):
    return (torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]).cuda()      # [groups, T] prefix mask


@functools.lru_cache(maxsize=None)
def _kv(lengths=tuple(LENGTHS), bound=BOUND):
    """K/V scattered to [groups, bound, INNER], random in the padding slots too; the prefix mask, the table, the packed
    rows."""
    g = torch.Generator().manual_seed(7 * bound + len(lengths))
    k = torch.randn(len(lengths), bound, INNER, generator=g).cuda()
    v = torch.randn(len(lengths), bound, INNER, generator=g).cuda()
    keep = _valid(lengths, bound)
    return k, v, keep, _cu(lengths), k[keep], v[keep]


def _q(groups, beams, Tq):
    g = torch.Generator().manual_seed(1000 * beams + Tq)
    return (torch.randn(groups * beams, Tq, INNER, generator=g) * 1.5).cuda()    # no 1/sqrt(d): scores reach 30


@pytest.mark.parametrize("Tq", [1, 2])
@pytest.mark.parametrize("beams", [1, 3, 10, 17])
def test_every_query_has_the_padded_bits(beams, Tq):
    from rqhip import ops
    k, v, keep, cu, kp, vp = _kv()
    q = _q(len(LENGTHS), beams, Tq)
    want = ops.t5_attention(q, k, v, H, key_mask=keep)
    out = ops.t5_attention_packed_beams(q, kp, vp, H, cu_k=cu, max_k=BOUND, beams=beams)
    assert out.shape == q.shape and out.dtype == torch.float32
    assert torch.equal(out, want)
    assert torch.equal(out, ops.t5_attention_packed_beams(q, kp, vp, H, cu_k=cu, max_k=BOUND, beams=beams))   # two runs
    if beams == 1:
        assert torch.equal(out, ops.t5_attention_packed(q, kp, vp, H, cu_k=cu, max_k=BOUND))


def test_the_largest_instantiation():
    from rqhip import ops
    lengths, bound, beams = (256, 1), 256, 10
    k, v, keep, cu, kp, vp = _kv(lengths, bound)
    q = _q(len(lengths), beams, 1)
    out = ops.t5_attention_packed_beams(q, kp, vp, H, cu_k=cu, max_k=bound, beams=beams)
    assert torch.equal(out, ops.t5_attention(q, k, v, H, key_mask=keep))
    # the single-key group: every beam returns that key's value row
    assert torch.equal(out[beams:], vp[256].expand(beams, 1, INNER))


def test_strided_q_and_kv_are_read_in_place():
    """q as a column slice of a wider tensor (a grouped projection's output), k and v as slices of one [N, 4 * INNER] tensor
    (cross_kv's grouped call for two blocks): the wrapper copies nothing and the bits are those of the dense tensors."""
    from rqhip import ops
    k, v, keep, cu, kp, vp = _kv()
    beams = 3
    q = _q(len(LENGTHS), beams, 2)
    wide_q = torch.randn(q.shape[0], q.shape[1], 3 * INNER, device="cuda")
    wide_q[..., INNER:2 * INNER] = q
    wide_kv = torch.randn(kp.shape[0], 4 * INNER, device="cuda")
    wide_kv[:, 2 * INNER:3 * INNER], wide_kv[:, 3 * INNER:] = kp, vp
    qs, ks, vs = wide_q[..., INNER:2 * INNER], wide_kv[:, 2 * INNER:3 * INNER], wide_kv[:, 3 * INNER:]
    assert not qs.is_contiguous() and not ks.is_contiguous() and ks.stride(0) == 4 * INNER
    seen = []
    handle = ops._lib.lib()

    class Spy:          # what reaches the C entry point: the views' own addresses and strides
        def rqhip_t5_attention_packed_beams(self, *a):
            seen.append(a[:5])
            return handle.rqhip_t5_attention_packed_beams(*a)

        def __getattr__(self, name):
            return getattr(handle, name)

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops._lib, "lib", lambda spy=Spy(): spy)
        out = ops.t5_attention_packed_beams(qs, ks, vs, H, cu_k=cu, max_k=BOUND, beams=beams)
    assert seen == [(qs.data_ptr(), 3 * INNER, ks.data_ptr(), vs.data_ptr(), 4 * INNER)]
    assert torch.equal(out, ops.t5_attention_packed_beams(q, kp, vp, H, cu_k=cu, max_k=BOUND, beams=beams))
    assert torch.equal(out, ops.t5_attention(q, k, v, H, key_mask=keep))


def test_against_the_operators_in_fp64():
    from rqhip import ops
    k, v, keep, cu, kp, vp = _kv()
    beams, Tq = 10, 2
    q = _q(len(LENGTHS), beams, Tq)
    out = ops.t5_attention_packed_beams(q, kp, vp, H, cu_k=cu, max_k=BOUND, beams=beams)
    rows = torch.arange(len(LENGTHS), device="cuda").repeat_interleave(beams)      # one K/V per query row
    attention_gate(f"packed beams {beams} x {Tq}", out, q, k[rows], v[rows], H, None, keep[rows][:, None, None, :])


def test_a_group_without_keys_gives_zeros():
    from rqhip import ops
    k, v, keep, cu, kp, vp = _kv()
    beams = 3
    q = _q(len(LENGTHS), beams, 2)
    full = ops.t5_attention_packed_beams(q, kp, vp, H, cu_k=cu, max_k=BOUND, beams=beams)
    lengths = [17, 0, 16, 5]                                  # group 1 loses its one key
    rows = torch.ones(kp.shape[0], dtype=torch.bool)
    rows[17] = False
    out = ops.t5_attention_packed_beams(q, kp[rows.cuda()], vp[rows.cuda()], H, cu_k=_cu(lengths), max_k=BOUND, beams=beams)
    assert not bool(out[beams:2 * beams].any())
    others = torch.ones(q.shape[0], dtype=torch.bool)
    others[beams:2 * beams] = False
    assert torch.equal(out[others.cuda()], full[others.cuda()]) and bool(full[beams:2 * beams].any())


def test_malformed_host_arguments_raise():
    from rqhip import ops
    from rqhip._lib import RqHipError
    k, v, keep, cu, kp, vp = _kv()
    beams = 3
    q = _q(len(LENGTHS), beams, 1)
    ok = dict(cu_k=cu, max_k=BOUND, beams=beams)
    ops.t5_attention_packed_beams(q, kp, vp, H, **ok)
    for bad in (dict(cu_k=cu.long()),                        # the table's dtype
                dict(cu_k=cu[:-1]),                          # the table's length: R // beams + 1
                dict(beams=5),                               # 12 rows
                dict(beams=0),
                dict(max_k=257)):                            # beyond the short kernel
        with pytest.raises(RqHipError):
            ops.t5_attention_packed_beams(q, kp, vp, H, **{**ok, **bad})
    with pytest.raises(RqHipError):
        ops.t5_attention_packed_beams(q, kp, vp[:-1], H, **ok)
    with pytest.raises(RqHipError):
        ops.t5_attention_packed_beams(q.double(), kp, vp, H, **ok)
    with pytest.raises(RqHipError):
        ops.t5_attention_packed_beams(q.cpu(), kp, vp, H, **ok)
