"""The "bf16" arithmetic of the fused T5 attention beyond 256 tokens on the device (rqhip_t5_attention_long_*_bf16 through
ops.t5_attention_long*(..., arith="bf16")): bf16 matrix operands, fp32 softmax and storage (contract: include/rqhip.h).

Reference: with bf(x) = x.to(bfloat16), the operator attention in fp64 on bf(q), bf(k), bf(v), bf(d_out) with P and dS
unrounded (retrieval_cases.attention_train_operators on the rounded tensors); `_ref_parts` restates it in fp64 to return
P~ = P o keep / (1 - p) and dS.  Noise yardstick: the fp32 long kernel on the same rounded tensors, per tensor
N = max|fp32 arm - ref64|.  Gates, elementwise, with u = 2^-8 (bf16's unit roundoff) and a slack factor 1 + 2^-6:
    out     |err| <= u (P~ @ |bf(v)|) + 4 N          d_v   |err| <= u (P~^T @ |bf(d_out)|) + 8 N
    d_q     |err| <= u (|dS| @ |bf(k)|) + 8 N        d_k   |err| <= u (|dS|^T @ |bf(q)|) + 8 N
    dtable  |err| <= 8 N (dS is not rounded on that path)
    lse     retrieval_cases.lse_gate against the reference on the rounded tensors; (m, l) reproduces lse.
The first term bounds the ONE rounding the arm adds (each rounded weight errs by at most u of itself, whatever chunk
maximum it was scaled by, and l sums unrounded weights); the factors 4 and 8 are those of test_gpu_t5_attention_long.py.
A tensor whose fp64 reference is exactly zero must be exactly zero.  The kernel is fed the UNROUNDED tensors: it rounds
them itself.  Every case runs twice and must give identical bits.  The lengths rest on the chunk C = 128 and the query
block Qb = 64: an odd count of 16-row tiles leaves half a 32-term group, 300 has a tail in both the chunk and the block.
The module's last lines are the largest |err| / gate per tensor (profiles/t5_attention_long_bf16.txt holds a run's)."""
import collections

import pytest
import torch

from retrieval_cases import (F32_MIN, _bias_module, _inputs, _padding, attention_train_operators, lse_gate, same_bits,
                             seed)

pytestmark = pytest.mark.gpu

C, QB = 128, 64
U = 2.0 ** -8
SLACK = 1.0 + 2.0 ** -6
FACTOR = dict(out=4, dq=8, dk=8, dv=8, dtable=8)
NAMES = ("out", "lse", "dq", "dk", "dv", "dtable")
LARGEST = collections.defaultdict(float)   # tensor name -> the largest |err| / gate of the module's cases
BF = dict(arith="bf16")


@pytest.fixture(scope="module", autouse=True)
def _largest_ratios():
    from rqhip import ops
    assert (ops.T5_ATTENTION_LONG_CHUNK, ops.T5_ATTENTION_LONG_QBLOCK) == (C, QB)
    yield
    print("\nlargest |err| / gate per tensor: " + ", ".join(f"{n} {r:.3f}" for n, r in sorted(LARGEST.items())))


def bf(x):
    return x.to(torch.bfloat16).float()


def _table(H, is_decoder, Tq, Tk, bias_seed=3):
    with torch.no_grad():
        table, offset = _bias_module(H, is_decoder, bias_seed).delta_table(Tq, Tk, 0)
    return table.detach().contiguous(), offset


def _d_out(R, Tq, H, s=0):
    return torch.randn(R, Tq, H * 64, generator=torch.Generator().manual_seed(1000 + s)).cuda()


def _keep(key_mask, causal, Tq, Tk):
    keep = None if key_mask is None else key_mask[:, None, None, :]
    if causal:
        tri = torch.ones(Tq, Tk, dtype=torch.bool, device="cuda").tril()[None, None]
        keep = tri if keep is None else keep & tri
    return keep


def _heads(x, H):
    return x.double().view(x.shape[0], x.shape[1], H, 64).transpose(1, 2)


def _rows(x):
    return x.transpose(1, 2).reshape(x.shape[0], x.shape[2], -1)


def _ref_parts(q, k, v, d_out, H, table, offset, keep, drop, p):
    """The reference's P~ = P o keep / (1 - p) and dS, [R, H, Tq, Tk] in fp64 (q, k, v, d_out already rounded)."""
    Tq, Tk = q.shape[1], k.shape[1]
    s = _heads(q, H) @ _heads(k, H).transpose(-1, -2)
    if table is not None:
        i = torch.arange(Tq, device=q.device)[:, None]
        j = torch.arange(Tk, device=q.device)[None, :]
        s = s + table.double()[(j - i) + offset].permute(2, 0, 1).unsqueeze(0)
    if keep is not None:
        s = s + (~keep).double() * F32_MIN
    P = torch.softmax(s, dim=-1)
    M = 1.0 if drop is None else drop.double() / (1 - p)
    dP = (_heads(d_out, H) @ _heads(v, H).transpose(-1, -2)) * M
    dS = P * (dP - (P * dP).sum(dim=-1, keepdim=True))
    return P * M, dS


def _run(q, k, v, H, d_out, **kw):
    from rqhip import ops
    with torch.no_grad():
        out, lse, ml = ops.t5_attention_long_fwd_train(q, k, v, H, **kw)
        return (out, lse) + tuple(ops.t5_attention_long_bwd(q, k, v, out, lse, ml, d_out, H, **kw)) + (ml,)


def _gate(case, tensor, got, fp32, ref64, bound):
    """One tensor's elementwise gate; `bound`: its first term without u (None: no rounding on that path)."""
    assert torch.isfinite(got).all(), f"{case} {tensor}"
    if not bool(ref64.any()):
        print(f"{case} {tensor}: the fp64 reference is exactly zero")
        assert not bool(got.any()), f"{case} {tensor}"
        return
    N = float((fp32.double() - ref64).abs().max())
    lim = torch.full_like(ref64, FACTOR[tensor] * N)
    if bound is not None:
        lim = lim + U * bound
    lim = lim * SLACK
    e = (got.double() - ref64).abs()
    over = e > lim
    ratio = float(torch.where(lim > 0, e / lim, torch.where(e > 0, float("inf"), 0.0).double()).max())
    LARGEST[tensor] = max(LARGEST[tensor], ratio)
    print(f"{case} {tensor}: max|err| {float(e.max()):.3e} N {N:.3e} largest |err| / gate {ratio:.3f}")
    assert not bool(over.any()), f"{case} {tensor}: {int(over.sum())} elements beyond the gate, ratio {ratio:.3f}"


def bf16_case(name, q, k, v, H, *, table=None, offset=0, key_mask=None, causal=False, p=0.0, seed=None, masked_row=None):
    """One shape through the bf16 fwd_train and bwd: the inference call's bits at p = 0, every gate, the fully masked row
    on its own, (m, l) against lse, a second run with identical bits.  Returns (out, lse, dq, dk, dv, dtable, ml)."""
    from rqhip import ops
    R, Tq, Tk = q.shape[0], q.shape[1], k.shape[1]
    d_out = _d_out(R, Tq, H)
    kw = dict(bias_by_delta=table, bias_offset=offset, key_mask=key_mask, causal=causal)
    got = _run(q, k, v, H, d_out, p=p, seed=seed, **kw, **BF)
    if p == 0:
        with torch.no_grad():
            assert same_bits(got[0], ops.t5_attention_long(q, k, v, H, **kw, **BF))
    qb, kb, vb, dob = bf(q), bf(k), bf(v), bf(d_out)
    fp32 = _run(qb, kb, vb, H, dob, p=p, seed=seed, **kw)          # the yardstick: the fp32 arm on the rounded tensors
    keep = _keep(key_mask, causal, Tq, Tk)
    drop = ops.t5_attention_dropout_keep(seed, R, H, Tq, Tk, p) if p > 0 else None
    ref64 = attention_train_operators(qb, kb, vb, H, table, offset, keep, drop, p, dob, torch.float64)
    Pt, dS = _ref_parts(qb, kb, vb, dob, H, table, offset, keep, drop, p)
    assert float((_rows(Pt @ _heads(vb, H)) - ref64[0]).abs().max()) <= 1e-11 * float(ref64[0].abs().max())
    bounds = dict(out=_rows(Pt @ _heads(vb, H).abs()), dv=_rows(Pt.transpose(-1, -2) @ _heads(dob, H).abs()),
                  dq=_rows(dS.abs() @ _heads(kb, H).abs()), dk=_rows(dS.abs().transpose(-1, -2) @ _heads(qb, H).abs()),
                  dtable=None)

    lse_gate(name, got[1], ref64[1])
    for n, x, x32, x64 in zip(NAMES, got, fp32, ref64):
        if n == "lse":
            continue
        assert (x is None) == (x64 is None)
        if x is not None:
            _gate(name, n, x, x32, x64, bounds[n])
    m, l = got[6][..., 0], got[6][..., 1]
    assert bool((l > 0).all()) and torch.isfinite(got[6]).all()
    lse_gate(f"{name}, from (m, l),", got[1], m.double() + torch.log(l.double()))
    if masked_row is not None and Tk > 1:     # every key masked: uniform P over ALL keys, dS != 0
        assert not bool(key_mask[masked_row].any()) and bool(ref64[2][masked_row].any())
        assert bool((m[masked_row] < -1e38).all())
        r = masked_row
        for n, x, x32, x64 in zip(NAMES, got[:5], fp32[:5], ref64[:5]):
            if n != "lse":
                _gate(f"{name}, the fully masked row,", n, x[r], x32[r], x64[r], bounds[n][r])
    again = _run(q, k, v, H, d_out, p=p, seed=seed, **kw, **BF)
    for x, y in zip(got, again):
        assert (x is None and y is None) or same_bits(x, y)
    return got


@pytest.mark.parametrize("T,H", [(1, 6), (15, 1), (16, 6), (17, 1), (31, 6), (32, 1), (33, 6), (C - 1, 1), (C, 6),
                                 (C + 1, 1), (257, 6), (300, 6)])
def test_encoder_self_attention(T, H):
    R = 3
    q, k, v, g = _inputs(R, T, R, T, H, 10 + T)
    table, offset = _table(H, False, T, T)
    bf16_case(f"encoder T={T} R={R} H={H}", q, k, v, H, table=table, offset=offset, key_mask=_padding(R, T, g),
              masked_row=1)


@pytest.mark.parametrize("padded", [False, True])
def test_causal_with_bias_table(padded):
    T, R, H = 257, 3, 6
    q, k, v, g = _inputs(R, T, R, T, H, 30 + T + padded)
    table, offset = _table(H, True, T, T)
    key_mask = _padding(R, T, g) if padded else None
    got = bf16_case(f"causal T={T} R={R} H={H} padded={padded}", q, k, v, H, table=table, offset=offset,
                    key_mask=key_mask, causal=True, masked_row=1 if padded else None)
    live = torch.ones(R, dtype=torch.bool, device="cuda") if key_mask is None else key_mask[:, 0]
    assert bool(live.any())
    assert torch.equal(got[0][live, 0], bf(v)[live, 0])   # the first query sees key 0 alone: weight exactly 1


@pytest.mark.parametrize("Tq,Tk,R,H", [(4, 1025, 2, 6), (QB + 1, 300, 3, 1), (300, 5, 3, 6), (17, 33, 3, 1),
                                       (33, 17, 3, 6)])
def test_cross_attention_without_a_table(Tq, Tk, R, H):
    q, k, v, g = _inputs(R, Tq, R, Tk, H, 50 + Tq)
    bf16_case(f"cross ({Tq}, {Tk}) R={R} H={H}", q, k, v, H, key_mask=_padding(R, Tk, g), masked_row=1)


DROP_SHAPES = {
    "encoder": dict(Tq=257, Tk=257, R=2, H=6, table=False, causal=False),
    "causal": dict(Tq=257, Tk=257, R=2, H=1, table=True, causal=True),
    "cross": dict(Tq=4, Tk=1025, R=2, H=6, table=None, causal=False),
}


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("form", sorted(DROP_SHAPES))
def test_dropout(form, p):
    from rqhip import ops
    c = DROP_SHAPES[form]
    Tq, Tk, R, H = c["Tq"], c["Tk"], c["R"], c["H"]
    q, k, v, g = _inputs(R, Tq, R, Tk, H, 70 + Tq)
    table, offset = (None, 0) if c["table"] is None else _table(H, c["table"], Tq, Tk)
    key_mask = _padding(R, Tk, g)
    s = seed((5 << 33) + 7)                                        # bits above the low 32
    got = bf16_case(f"dropout {form} p={p}", q, k, v, H, table=table, offset=offset, key_mask=key_mask,
                    causal=c["causal"], p=p, seed=s, masked_row=1)
    with torch.no_grad():
        other = ops.t5_attention_long_fwd_train(q, k, v, H, bias_by_delta=table, bias_offset=offset, key_mask=key_mask,
                                                causal=c["causal"], p=p, seed=seed(int(s) + (1 << 32)), **BF)[0]
    assert not torch.equal(other, got[0])


def test_masks_that_padding_does_not_make():
    R, H, T = 3, 6, 300
    q, k, v, g = _inputs(R, T, R, T, H, 61)
    table, offset = _table(H, False, T, T)
    key_mask = torch.ones(R, T, dtype=torch.bool, device="cuda")
    key_mask[0] = False                 # every key masked: the average of V
    key_mask[1, :C] = False             # the whole first chunk masked, later keys live: the rescale away from finfo.min
    key_mask[2, 100:] = False           # live keys in the first chunk only
    got = bf16_case("special masks", q, k, v, H, table=table, offset=offset, key_mask=key_mask, masked_row=0)
    assert not bool(got[3][1, :C].any()) and not bool(got[4][1, :C].any())   # masked keys of a live row: weight exactly 0
    assert not bool(got[3][2, 100:].any()) and not bool(got[4][2, 100:].any())


def test_one_live_key_gives_zero_dq_and_dk_exactly():
    R, H, T = 2, 6, 257
    q, k, v, g = _inputs(R, T, R, T, H, 65)
    table, offset = _table(H, False, T, T)
    key_mask = torch.zeros(R, T, dtype=torch.bool, device="cuda")
    key_mask[0, 200] = True             # in the second chunk
    key_mask[1, 5] = True
    got = bf16_case("one live key", q, k, v, H, table=table, offset=offset, key_mask=key_mask)
    assert not bool(got[2].any()) and not bool(got[3].any())       # P = 1 on one key: D = dP, dS = 0
    assert torch.equal(got[0][0], bf(v)[0, 200].expand(T, -1)) and torch.equal(got[0][1], bf(v)[1, 5].expand(T, -1))


def test_the_limit_2048():
    R, H, T = 1, 1, 2048
    q, k, v, g = _inputs(R, T, R, T, H, 81)
    table, offset = _table(H, False, T, T)
    key_mask = torch.ones(R, T, dtype=torch.bool, device="cuda")
    key_mask[0, 2000:] = False
    bf16_case("limit T=2048", q, k, v, H, table=table, offset=offset, key_mask=key_mask)


def test_cross_attention_one_query_ten_beams_per_group_inference():
    from rqhip import ops
    Rk, beams, H, Tk = 2, 10, 6, 257
    q, k, v, g = _inputs(Rk * beams, 1, Rk, Tk, H, 41)
    key_mask = _padding(Rk, Tk, g)
    key_mask[1, 200:] = True                      # no wholly masked group here: a padded tail and an open tail
    key_mask[1, :130] = False
    with torch.no_grad():
        out = ops.t5_attention_long(q, k, v, H, key_mask=key_mask, **BF)
        again = ops.t5_attention_long(q, k, v, H, key_mask=key_mask, **BF)
        kx, vx, mx = (t.repeat_interleave(beams, dim=0) for t in (k, v, key_mask))
        fp32 = ops.t5_attention_long(bf(q), bf(k), bf(v), H, key_mask=key_mask)
        train = ops.t5_attention_long_fwd_train(q, kx, vx, H, key_mask=mx, **BF)[0]
    keep = mx[:, None, None, :]
    d_out = _d_out(Rk * beams, 1, H)
    out64 = attention_train_operators(bf(q), bf(kx), bf(vx), H, None, 0, keep, None, 0.0, bf(d_out), torch.float64)[0]
    Pt, _ = _ref_parts(bf(q), bf(kx), bf(vx), bf(d_out), H, None, 0, keep, None, 0.0)
    _gate("cross (1, 257) x 10 beams", "out", out, fp32, out64, _rows(Pt @ _heads(bf(vx), H).abs()))
    assert same_bits(out, again)
    assert same_bits(out, train)                  # the beams of a group against one K/V per row
    # a row's bits do not depend on the number of beams or of groups: one beam of one group alone
    with torch.no_grad():
        alone = ops.t5_attention_long(q[13:14], k[1:2], v[1:2], H, key_mask=key_mask[1:2], **BF)
    assert same_bits(alone, out[13:14])


def test_row_strides_column_slices_of_one_buffer():
    from rqhip import ops
    R, H, T = 2, 6, 257
    hd = H * 64
    q, k, v, g = _inputs(R, T, R, T, H, 91)
    buf = torch.cat([q, k, v], dim=-1)
    qs, ks, vs = buf[..., :hd], buf[..., hd:2 * hd], buf[..., 2 * hd:]
    assert not qs.is_contiguous() and qs.stride(1) == 3 * hd
    table, offset = _table(H, False, T, T)
    key_mask = _padding(R, T, g)
    kw = dict(bias_by_delta=table, bias_offset=offset, key_mask=key_mask, **BF)
    d_out = _d_out(R, T, H)
    want = _run(q, k, v, H, d_out, **kw)

    def no_copy(t):
        raise AssertionError("a strided operand was copied")

    saved = ops._aligned16
    ops._aligned16 = no_copy
    try:
        got = _run(qs, ks, vs, H, d_out, **kw)
        with torch.no_grad():
            inference = ops.t5_attention_long(qs, ks, vs, H, **kw)
    finally:
        ops._aligned16 = saved
    for x, y in zip(got, want):
        assert same_bits(x, y)
    assert same_bits(inference, want[0])
    # the kernel's rounding is torch's: tensors rounded beforehand give the same bits
    for x, y in zip(_run(bf(q), bf(k), bf(v), H, bf(d_out), **kw), want):
        assert same_bits(x, y)


def test_arith_fp32_is_the_call_without_the_keyword_and_bf16_is_another_arithmetic():
    R, H, T = 2, 1, 300
    q, k, v, g = _inputs(R, T, R, T, H, 97)
    table, offset = _table(H, False, T, T)
    kw = dict(bias_by_delta=table, bias_offset=offset, key_mask=_padding(R, T, g))
    d_out = _d_out(R, T, H)
    from rqhip import ops
    want = _run(q, k, v, H, d_out, **kw)
    for x, y in zip(_run(q, k, v, H, d_out, arith="fp32", **kw), want):
        assert same_bits(x, y)
    with torch.no_grad():
        assert same_bits(ops.t5_attention_long(q, k, v, H, arith="fp32", **kw), want[0])
    other = _run(q, k, v, H, d_out, **kw, **BF)
    assert not same_bits(other[0], want[0]) and not same_bits(other[2], want[2])
