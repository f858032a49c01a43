"""The fused T5 attention beyond 256 tokens on the device (csrc/t5_attention_long.hip through ops.t5_attention_long,
ops.t5_attention_long_fwd_train and ops.t5_attention_long_bwd) against the project's operator references in fp64 and fp32
(retrieval_cases.attention_operators / attention_train_operators).

Gates, the project's own, without floors: e = max|a - a64| / max|a64| per tensor; out: e_kernel <= 4 e_torch; dq, dk, dv,
dtable: e_kernel <= 8 e_torch; lse: lse_gate (1e-6).  Every case runs twice and must give identical bits.  With the
kernel's chunk C = 128 keys and query block Qb = 64 rows the lengths are the smallest at which a tiled kernel can go
wrong: one chunk (1, 17, C - 1, C, C + 1 -- the last is the first with a tail chunk), two whole chunks, two and one key,
the first length beyond the short kernel (257), a length with a tail in both the chunk and the query block (300), and
the limit (2048).  Every ratio is printed; the module's last lines are the largest ratio per tensor
(profiles/t5_attention_long.txt holds a run's)."""
import collections

import pytest
import torch

from retrieval_cases import (_bias_module, _inputs, _padding, attention_operators, attention_train_operators, err, gate,
                             lse_gate, same_bits, seed)

pytestmark = pytest.mark.gpu

C, QB = 128, 64
LARGEST = collections.defaultdict(float)   # tensor name -> the largest e_kernel / e_torch of the module's cases


@pytest.fixture(scope="module", autouse=True)
def _largest_ratios():
    from rqhip import ops
    assert (ops.T5_ATTENTION_LONG_CHUNK, ops.T5_ATTENTION_LONG_QBLOCK) == (C, QB)
    yield
    print("\nlargest e_kernel / e_torch per tensor: " + ", ".join(f"{n} {r:.2f}" for n, r in sorted(LARGEST.items())))


def _gate(case, tensor, got, ref32, ref64, factor):
    """retrieval_cases.gate without a floor, and the ratio kept for the module's summary."""
    if bool(ref64.any()):
        e_kernel, e_ref = err(got, ref64), err(ref32, ref64)
        ratio = e_kernel / e_ref if e_ref > 0 else (0.0 if e_kernel == 0 else float("inf"))
        LARGEST[tensor] = max(LARGEST[tensor], ratio)
    gate(f"{case} {tensor}", got, ref32, ref64, factor, floor=0.0)


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


def _run(q, k, v, H, d_out, **kw):
    from rqhip import ops
    with torch.no_grad():
        out, lse, ml = ops.t5_attention_long_fwd_train(q, k, v, H, **kw)
        return (out, lse) + tuple(ops.t5_attention_long_bwd(q, k, v, out, lse, ml, d_out, H, **kw)) + (ml,)


def long_case(name, q, k, v, H, *, table=None, offset=0, key_mask=None, causal=False, p=0.0, seed=None, masked_row=None,
              short=False):
    """One shape through fwd_train and bwd: the inference call's bits at p = 0, every gate, the fully masked row on its
    own, (m, l) against lse, and a second run with identical bits.  `short`: also the same gates with the short kernel's
    tensors in the operators' place.  Returns (out, lse, dq, dk, dv, dtable, ml, d_out, ref64)."""
    from rqhip import ops
    R, Tq, Tk = q.shape[0], q.shape[1], k.shape[1]
    d_out = _d_out(R, Tq, H)
    kw = dict(bias_by_delta=table, bias_offset=offset, key_mask=key_mask, causal=causal)
    got = _run(q, k, v, H, d_out, p=p, seed=seed, **kw)
    if p == 0:
        with torch.no_grad():
            assert same_bits(got[0], ops.t5_attention_long(q, k, v, H, **kw))
    keep = _keep(key_mask, causal, Tq, Tk)
    drop = ops.t5_attention_dropout_keep(seed, R, H, Tq, Tk, p) if p > 0 else None
    ref64 = attention_train_operators(q, k, v, H, table, offset, keep, drop, p, d_out, torch.float64)
    ref32 = attention_train_operators(q, k, v, H, table, offset, keep, drop, p, d_out, torch.float32)
    names = ("out", "lse", "dq", "dk", "dv", "dtable")
    factors = dict(out=4, dq=8, dk=8, dv=8, dtable=8)

    def gates(label, other):
        for n, x, x32, x64 in zip(names, got, other, ref64):
            if n == "lse":
                continue
            assert (x is None) == (x64 is None)
            if x is not None:
                _gate(label, n, x, x32, x64, factors[n])

    lse_gate(name, got[1], ref64[1])
    gates(name, ref32)
    m, l = got[6][..., 0], got[6][..., 1]
    assert bool((l > 0).all()) and torch.isfinite(got[6]).all()
    lse_gate(f"{name}, from (m, l),", got[1], m.double() + torch.log(l.double()))
    if masked_row is not None and Tk > 1:     # every key masked: uniform P over ALL keys, dS != 0
        assert not bool(key_mask[masked_row].any()) and bool(ref64[2][masked_row].any())
        assert bool((m[masked_row] < -1e38).all())
        for n, x, x32, x64 in zip(names, got[:5], ref32[:5], ref64[:5]):
            if n != "lse":
                _gate(f"{name}, the fully masked row,", n, x[masked_row], x32[masked_row], x64[masked_row], factors[n])
    if short:
        assert p == 0 and Tq <= 256 and Tk <= 256
        with torch.no_grad():
            s_out, s_lse = ops.t5_attention_fwd_train(q, k, v, H, **kw)
            s = (s_out, s_lse) + tuple(ops.t5_attention_bwd(q, k, v, s_out, s_lse, d_out, H, **kw))
        gates(f"{name} against the short kernel", s)
    again = _run(q, k, v, H, d_out, p=p, seed=seed, **kw)
    for x, y in zip(got, again):
        assert (x is None and y is None) or same_bits(x, y)
    return got + (d_out, ref64)


def _encoder(T, R, H, s, **kw):
    q, k, v, g = _inputs(R, T, R, T, H, s)
    table, offset = _table(H, False, T, T)
    return long_case(f"encoder T={T} R={R} H={H}", q, k, v, H, table=table, offset=offset, key_mask=_padding(R, T, g),
                     masked_row=1 if R > 1 else None, **kw)


@pytest.mark.parametrize("T,R,H", [(257, 3, 6), (2 * C, 2, 1), (2 * C + 1, 2, 1), (300, 5, 6)])
def test_encoder_self_attention_beyond_one_chunk(T, R, H):
    _encoder(T, R, H, 10 + T)


@pytest.mark.parametrize("T,R,H", [(1, 3, 6), (17, 3, 6), (C - 1, 2, 1), (C, 3, 6), (C + 1, 2, 1)])
def test_encoder_self_attention_single_chunk_group_also_against_the_short_kernel(T, R, H):
    _encoder(T, R, H, 20 + T, short=True)


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("T,R,H", [(257, 3, 6), (2 * C + 1, 2, 1)])
def test_causal_with_bias_table(T, R, H, padded):
    q, k, v, g = _inputs(R, T, R, T, H, 30 + T + padded)
    table, offset = _table(H, True, T, T)
    key_mask = _padding(R, T, g) if padded else None
    got = long_case(f"causal T={T} R={R} H={H} padded={padded}", q, k, v, H, table=table, offset=offset, key_mask=key_mask,
                    causal=True, masked_row=1 if padded else None)
    live = torch.ones(R, dtype=torch.bool, device="cuda") if key_mask is None else key_mask[:, 0]
    assert bool(live.any())
    assert torch.equal(got[0][live, 0], v[live, 0])     # the first query sees key 0 alone: weight exactly 1


def test_cross_attention_one_query_ten_beams_per_group_inference():
    from rqhip import ops
    Rk, beams, H, Tk = 2, 10, 6, 257
    q, k, v, g = _inputs(Rk * beams, 1, Rk, Tk, H, 41)
    key_mask = _padding(Rk, Tk, g)
    key_mask[1, 200:] = True                      # no wholly masked group here: a padded tail and an open tail
    key_mask[1, :130] = False
    with torch.no_grad():
        out = ops.t5_attention_long(q, k, v, H, key_mask=key_mask)
        again = ops.t5_attention_long(q, k, v, H, key_mask=key_mask)
    kx, vx, mx = (t.repeat_interleave(beams, dim=0) for t in (k, v, key_mask))
    keep = mx[:, None, None, :]
    out64 = attention_operators(q, kx, vx, H, None, keep, torch.float64)
    out32 = attention_operators(q, kx, vx, H, None, keep, torch.float32)
    _gate("cross (1, 257) x 10 beams", "out", out, out32, out64, 4)
    assert same_bits(out, again)
    # a row's bits do not depend on the number of beams or of groups: one beam of one group alone
    with torch.no_grad():
        alone = ops.t5_attention_long(q[13:14], k[1:2], v[1:2], H, key_mask=key_mask[1:2])
    assert same_bits(alone, out[13:14])


@pytest.mark.parametrize("Tq,Tk,R,H", [(4, 1025, 2, 6), (QB + 1, 300, 3, 1), (300, 5, 3, 6)])
def test_cross_attention_without_a_table(Tq, Tk, R, H):
    q, k, v, g = _inputs(R, Tq, R, Tk, H, 50 + Tq)
    long_case(f"cross ({Tq}, {Tk}) R={R} H={H}", q, k, v, H, key_mask=_padding(R, Tk, g), masked_row=1)


def test_masks_that_padding_does_not_make():
    R, H, T = 3, 6, 300
    q, k, v, g = _inputs(R, T, R, T, H, 61)
    table, offset = _table(H, False, T, T)
    key_mask = torch.ones(R, T, dtype=torch.bool, device="cuda")
    key_mask[0] = False                 # every key masked: the average of V
    key_mask[1, :C] = False             # the whole first chunk masked, later keys live: the rescale away from finfo.min
    key_mask[2, 100:] = False           # live keys in the first chunk only
    got = long_case("special masks", q, k, v, H, table=table, offset=offset, key_mask=key_mask, masked_row=0)
    d_out, ref64 = got[7], got[8]
    # the fully masked row's reference IS the average of V (long_case gated the row on its own)
    mean_v = v[0].double().mean(dim=0, keepdim=True).expand(T, -1)
    assert err(ref64[0][0], mean_v) <= 1e-12
    keep = key_mask[:, None, None, :]
    ref32 = attention_train_operators(q, k, v, H, table, offset, keep, None, 0.0, d_out, torch.float32)
    for row, what in ((1, "first chunk masked"), (2, "first chunk only")):
        for i, n, factor in ((0, "out", 4), (2, "dq", 8), (3, "dk", 8), (4, "dv", 8)):
            _gate(f"special masks, row {row} ({what}),", n, got[i][row], ref32[i][row], ref64[i][row], factor)
    assert not bool(got[3][1, :C].any()) and not bool(got[4][1, :C].any())   # masked keys of a live row: weight exactly 0


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
    s = seed((5 << 33) + 7) if form != "causal" else seed(12345)        # bits above the low 32
    got = long_case(f"dropout {form} p={p}", q, k, v, H, table=table, offset=offset, key_mask=key_mask, causal=c["causal"],
                    p=p, seed=s, masked_row=1)
    with torch.no_grad():
        other = ops.t5_attention_long_fwd_train(q, k, v, H, bias_by_delta=table, bias_offset=offset, key_mask=key_mask,
                                                causal=c["causal"], p=p, seed=seed(int(s) + (1 << 32)))[0]
    assert not torch.equal(other, got[0])


def test_the_limit_2048():
    R, H, T = 1, 1, 2048
    q, k, v, g = _inputs(R, T, R, T, H, 81)
    table, offset = _table(H, False, T, T)
    key_mask = torch.ones(R, T, dtype=torch.bool, device="cuda")
    key_mask[0, 2000:] = False
    long_case("limit T=2048", q, k, v, H, table=table, offset=offset, key_mask=key_mask)


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
    kw = dict(bias_by_delta=table, bias_offset=offset, key_mask=key_mask)
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


def test_bias_table_longer_than_needed_with_nan_padding_rows():
    R, H, T = 2, 6, 257
    q, k, v, g = _inputs(R, T, R, T, H, 95)
    table, offset = _table(H, False, T, T)
    nan = torch.full((5, H), float("nan"), device="cuda")
    padded = torch.cat([nan, table, nan, nan[:2]], dim=0)
    key_mask = _padding(R, T, g)
    d_out = _d_out(R, T, H)
    want = _run(q, k, v, H, d_out, bias_by_delta=table, bias_offset=offset, key_mask=key_mask)
    got = _run(q, k, v, H, d_out, bias_by_delta=padded, bias_offset=offset + 5, key_mask=key_mask)
    for i in (0, 1, 2, 3, 4, 6):
        assert same_bits(got[i], want[i])
    assert got[5].shape == padded.shape
    assert same_bits(got[5][5:5 + table.shape[0]], want[5])
    assert not bool(got[5][:5].any()) and not bool(got[5][5 + table.shape[0]:].any())


def test_peak_memory_stays_below_one_score_tensor():
    from rqhip import ops
    R, H, T = 2, 2, 1024
    q, k, v, g = _inputs(R, T, R, T, H, 99)
    table, offset = _table(H, False, T, T)
    key_mask = _padding(R, T, g)
    d_out = _d_out(R, T, H)
    kw = dict(bias_by_delta=table, bias_offset=offset, key_mask=key_mask)
    _run(q, k, v, H, d_out, **kw)                 # the LDS attribute and the allocator's first blocks
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    got = _run(q, k, v, H, d_out, **kw)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    one_score_tensor = R * H * T * T * 4
    held = sum(t.numel() * 4 for t in got if t is not None) + ops.t5_attention_long_bwd_workspace_bytes(R, H, T, T)
    print(f"peak rise {rise} bytes, outputs and workspace {held} bytes, one score tensor {one_score_tensor} bytes")
    assert rise < one_score_tensor
