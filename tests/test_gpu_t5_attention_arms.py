"""Every code path csrc/t5_attention.hip picks from a call's shape, on the GPU, against the operators in fp64: the key
tiles a lane holds (MT = 1 | 6 | 16, edges Tk = 16|17 and 96|97), the forward's one-wave arm, the backward's own
workgroup size and its staging buffer of max(Tq, Tk) rows, the causal mask beyond one 16-key tile in both of the
backward's register layouts, the dense form at past > 0, the bias gradient's diagonals at Tq != Tk, dropout on every arm,
and the row strides, mask types and table lengths ops.py passes through.  A test's name says which gap of the kernel-level
tests it closes:

  gap1  the MT edges Tk = 16, 17, 96, 97, forward and backward
  gap2  the causal mask across a 16-key tile (pass 1's and the key-major pass 2's comparison)
  gap3  causal with a key mask, causal with dropout
  gap4  the dense form with past > 0 and Tq > 1
  gap5  the forward's one-wave arm with more than one query tile
  gap6  the backward with Tq > Tk, and MT = 1 on four waves
  gap7  the bias gradient with Tq != Tk
  gap8  dropout on the MT = 1 and MT = 16 arms
  gap9  sliced and unaligned inputs, uint8 and strided key masks, a bias table longer than the call needs

References and gates are those of test_gpu_t5_attention.py (retrieval_cases.attention_gate: e_kernel <= 4 e_torch) and of
test_gpu_t5_attention_backward.py (retrieval_cases.attention_train_case: 4 for out, 8 for dq, dk, dv and dtable, lse at
1e-6, exact zeros, a second run with the same bits, the inference kernel's bits at p = 0).  Measured ratios:
profiles/retrieval_generate.txt (the inference kernel) and profiles/retrieval_train_step.txt (the training pair)."""
import numpy as np
import pytest
import torch

from retrieval_cases import (_bias_module, _inputs, _padding, attention_gate, attention_train_case, same_bits,
                             seed as _seed)

pytestmark = pytest.mark.gpu

R_SELF = 5


def _self_inputs(T, H, causal):
    """A self-attention call as the two older modules draw it: q, k, v, the bias module, its table and offset, padding."""
    if causal:
        q, k, v, g = _inputs(R_SELF, T, R_SELF, T, H, 7 * T + H)
        att = _bias_module(H, True, T)
    else:
        q, k, v, g = _inputs(R_SELF, T, R_SELF, T, H, 100 * T + H)
        att = _bias_module(H, False, T + H)
    keep = _padding(R_SELF, T, g)
    with torch.no_grad():
        table, offset = att.delta_table(T, T, 0)
    return q, k, v, att, table, offset, keep


def _tril(Tq, Tk, past=0):
    """[1, 1, Tq, Tk]: key j <= query i + past."""
    return (torch.arange(Tk, device="cuda")[None, :] <= torch.arange(Tq, device="cuda")[:, None] + past)[None, None]


def _is_average_of_v(out_rows, v_row):
    """Every key masked: the uniform average of V, as with the operators."""
    want = v_row.mean(dim=0, keepdim=True).expand(out_rows.shape[-2], -1).expand_as(out_rows)
    np.testing.assert_allclose(out_rows.cpu().numpy(), want.cpu().numpy(), rtol=0, atol=1e-5)


def _nan_padded(table, rows=3):
    pad = torch.full((rows, table.shape[1]), float("nan"), device=table.device)
    return torch.cat([pad, table, pad], dim=0)


# ---- A. the inference kernel


@pytest.mark.parametrize("T,H", [(15, 6), (16, 6), (17, 6), (96, 6), (97, 6), (112, 6), (16, 1), (17, 1)])
def test_gap1_encoder_attention_at_the_mt_edges(T, H):
    from rqhip import ops
    q, k, v, att, table, offset, keep = _self_inputs(T, H, False)
    kw = dict(bias_by_delta=table, bias_offset=offset, key_mask=keep)
    with torch.no_grad():
        out = ops.t5_attention(q, k, v, H, **kw)
        attention_gate(f"gap1 encoder T={T} H={H}", out, q, k, v, H, att.compute_bias(T, T), keep[:, None, None, :])
        _is_average_of_v(out[1], v[1])
        again = ops.t5_attention(q, k, v, H, **kw)
    assert same_bits(again, out)


@pytest.mark.parametrize("T", [16, 17, 33, 97])
def test_gap2_causal_attention_across_key_tiles(T):
    from rqhip import ops
    H = 6
    q, k, v, att, table, offset, _ = _self_inputs(T, H, True)
    kw = dict(bias_by_delta=table, bias_offset=offset, causal=True)
    with torch.no_grad():
        out = ops.t5_attention(q, k, v, H, **kw)
        attention_gate(f"gap2 causal T={T} H={H}", out, q, k, v, H, att.compute_bias(T, T), _tril(T, T))
        assert torch.equal(out[:, 0], v[:, 0])              # the first query sees one key: exact
        again = ops.t5_attention(q, k, v, H, **kw)
    assert same_bits(again, out)


def test_gap3_causal_attention_with_a_padding_mask():
    from rqhip import ops
    T, H = 33, 6
    q, k, v, att, table, offset, keep = _self_inputs(T, H, True)
    kw = dict(bias_by_delta=table, bias_offset=offset, causal=True, key_mask=keep)
    with torch.no_grad():
        out = ops.t5_attention(q, k, v, H, **kw)
        attention_gate(f"gap3 causal and padding T={T} H={H}", out, q, k, v, H, att.compute_bias(T, T),
                       _tril(T, T) & keep[:, None, None, :])
        assert torch.equal(out[0, 0], v[0, 0])              # row 0 keeps every key: its first query sees one
        _is_average_of_v(out[1], v[1])                      # row 1: every score got the one addend, causal or not
        again = ops.t5_attention(q, k, v, H, **kw)
    assert same_bits(again, out)


@pytest.mark.parametrize("Tk,beams,Tq", [(9, 10, 3), (16, 10, 5)])
def test_gap5_one_wave_arm_with_several_query_tiles(Tk, beams, Tq):
    from rqhip import ops
    B, H = 6, 6
    assert Tk <= 16 < beams * Tq
    q, k, v, g = _inputs(B * beams, Tq, B, Tk, H, 31 * beams + Tq + Tk)
    keep = _padding(B, Tk, g)
    kx, vx = k.repeat_interleave(beams, 0), v.repeat_interleave(beams, 0)
    with torch.no_grad():
        out = ops.t5_attention(q, k, v, H, key_mask=keep)
        attention_gate(f"gap5 cross Tk={Tk} beams={beams} Tq={Tq}", out, q, kx, vx, H, None,
                       keep.repeat_interleave(beams, 0)[:, None, None, :])
        _is_average_of_v(out[beams:2 * beams], v[1])        # the beams of K/V group 1
        unmasked = ops.t5_attention(q, k, v, H)
        attention_gate(f"gap5 cross Tk={Tk} beams={beams} Tq={Tq} no mask", unmasked, q, kx, vx, H, None, None)
        again = ops.t5_attention(q, k, v, H, key_mask=keep)
        again_unmasked = ops.t5_attention(q, k, v, H)
    assert same_bits(again, out) and same_bits(again_unmasked, unmasked)


@pytest.mark.parametrize("Tq,past,Tk", [(3, 14, 17), (5, 92, 97)])
def test_gap4_dense_form_with_past_and_several_queries(Tq, past, Tk):
    from rqhip import ops
    H = 6
    q, k, v, _ = _inputs(R_SELF, Tq, R_SELF, Tk, H, 13 * past + Tq)
    att = _bias_module(H, True, past)
    with torch.no_grad():
        table, offset = att.delta_table(Tq, Tk, past)
        kw = dict(bias_by_delta=table, bias_offset=offset, causal=True, past=past)
        out = ops.t5_attention(q, k, v, H, **kw)
        attention_gate(f"gap4 dense Tq={Tq} past={past} Tk={Tk}", out, q, k, v, H, att.compute_bias(Tq, Tk, past),
                       _tril(Tq, Tk, past))
        again = ops.t5_attention(q, k, v, H, **kw)
    assert same_bits(again, out)


@pytest.mark.parametrize("causal", [False, True], ids=["encoder", "causal"])
def test_gap9_longer_bias_table_in_the_inference_kernel(causal):
    from rqhip import ops
    T, H = (17, 6) if causal else (33, 6)
    q, k, v, att, table, offset, keep = _self_inputs(T, H, causal)
    kw = dict(causal=True) if causal else dict(key_mask=keep)
    with torch.no_grad():
        want = ops.t5_attention(q, k, v, H, bias_by_delta=table, bias_offset=offset, **kw)
        out = ops.t5_attention(q, k, v, H, bias_by_delta=_nan_padded(table), bias_offset=offset + 3, **kw)
    assert torch.isfinite(out).all() and same_bits(out, want)


# ---- B. the training pair


@pytest.mark.parametrize("T", [16, 96, 97, 112])
def test_gap1_encoder_backward_at_the_mt_edges(T):
    H = 6
    q, k, v, att, table, offset, keep = _self_inputs(T, H, False)
    attention_train_case(f"gap1 encoder T={T} H={H}", q, k, v, H, table=table, offset=offset, key_mask=keep,
                         seed_d_out=T + H, masked_row=1)


@pytest.mark.parametrize("T,H", [(16, 6), (17, 1), (17, 6), (33, 6), (97, 6)])
def test_gap2_causal_backward_across_key_and_query_tiles(T, H):
    q, k, v, att, table, offset, _ = _self_inputs(T, H, True)
    attention_train_case(f"gap2 causal T={T} H={H}", q, k, v, H, table=table, offset=offset, causal=True, seed_d_out=T)


def test_gap3_causal_backward_with_a_padding_mask():
    T, H = 33, 6
    q, k, v, att, table, offset, keep = _self_inputs(T, H, True)
    attention_train_case(f"gap3 causal and padding T={T} H={H}", q, k, v, H, table=table, offset=offset, causal=True,
                         key_mask=keep, seed_d_out=T, masked_row=1)


def _cross(Tq, Tk, H=6, R=6):
    q, k, v, g = _inputs(R, Tq, R, Tk, H, 31 + Tq + Tk + H)
    return q, k, v, _padding(R, Tk, g)


@pytest.mark.parametrize("Tq,Tk", [(17, 16), (33, 3), (81, 4), (16, 17), (16, 16)])
def test_gap6_backward_with_tq_above_tk_and_both_workgroup_sizes(Tq, Tk):
    """(17, 16): MT = 1 on four waves; (33, 3), (81, 4): the staging buffer is sized by Tq; (16, 17) | (16, 16): the two
    sides of the backward's one-wave condition."""
    H = 6
    q, k, v, keep = _cross(Tq, Tk)
    attention_train_case(f"gap6 cross Tq={Tq} Tk={Tk} H={H}", q, k, v, H, key_mask=keep, seed_d_out=Tk, masked_row=1)


@pytest.mark.parametrize("Tq,Tk", [(5, 37), (16, 97)])
def test_gap7_bias_gradient_with_tq_below_tk(Tq, Tk):
    H = 6
    q, k, v, _ = _inputs(R_SELF, Tq, R_SELF, Tk, H, 100 * Tk + Tq)
    att = _bias_module(H, False, Tq + Tk)
    with torch.no_grad():
        table, offset = att.delta_table(Tq, Tk, 0)
    assert table.shape[0] == Tq + Tk - 1
    attention_train_case(f"gap7 bias Tq={Tq} Tk={Tk} H={H}", q, k, v, H, table=table, offset=offset, seed_d_out=Tq)


HIGH_SEED = (0x5DEECE66 << 32) | 0x0000002B      # bits above the low 32: the hash's second round sees them


def _dropout_case(name, q, k, v, H, p, seed, other_seed, *, table=None, offset=0, key_mask=None, causal=False, **case):
    """The training case with keep from ops.t5_attention_dropout_keep(seed, ...); another seed gives another `out`."""
    from rqhip import ops
    out = attention_train_case(f"{name} p={p}", q, k, v, H, table=table, offset=offset, key_mask=key_mask, causal=causal,
                               p=p, seed=_seed(seed), **case)[0]
    with torch.no_grad():
        other, _ = ops.t5_attention_fwd_train(q, k, v, H, bias_by_delta=table, bias_offset=offset, key_mask=key_mask,
                                              causal=causal, p=p, seed=_seed(other_seed))
    assert not torch.equal(other, out)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("T", [16, 97])
def test_gap8_encoder_dropout_on_the_mt1_and_mt16_arms(T, p):
    H = 6
    q, k, v, att, table, offset, keep = _self_inputs(T, H, False)
    seed = HIGH_SEED if T == 97 else 77 + T
    _dropout_case(f"gap8 encoder T={T} H={H}", q, k, v, H, p, seed, seed + 1, table=table, offset=offset, key_mask=keep,
                  seed_d_out=T + H, masked_row=1)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("T", [17, 33])
def test_gap3_causal_dropout(T, p):
    H = 6
    q, k, v, att, table, offset, _ = _self_inputs(T, H, True)
    _dropout_case(f"gap3 causal T={T} H={H}", q, k, v, H, p, 177 + T, 178 + T, table=table, offset=offset, causal=True,
                  seed_d_out=T)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_gap8_cross_dropout_on_mt1_with_four_waves(p):
    Tq, Tk, H = 17, 16, 6
    q, k, v, keep = _cross(Tq, Tk)
    _dropout_case(f"gap8 cross Tq={Tq} Tk={Tk} H={H}", q, k, v, H, p, -3, 4, key_mask=keep, seed_d_out=Tk, masked_row=1)


def test_gap9_longer_bias_table_in_the_backward():
    from rqhip import ops
    T, H = 33, 6
    q, k, v, att, table, offset, keep = _self_inputs(T, H, False)
    d_out = torch.randn(R_SELF, T, H * 64, generator=torch.Generator().manual_seed(9)).to("cuda")

    def run(tab, off):
        kw = dict(bias_by_delta=tab, bias_offset=off, key_mask=keep)
        out, lse = ops.t5_attention_fwd_train(q, k, v, H, **kw)
        return (out, lse) + tuple(ops.t5_attention_bwd(q, k, v, out, lse, d_out, H, **kw))

    with torch.no_grad():
        want, got = run(table, offset), run(_nan_padded(table), offset + 3)
    assert want[5].shape[0] == 2 * T - 1 and got[5].shape[0] == 2 * T - 1 + 6
    for x, y in zip(got[:5], want[:5]):
        assert torch.isfinite(x).all() and same_bits(x, y)
    assert same_bits(got[5][3:-3], want[5]) and bool(want[5].any())
    assert not bool(got[5][:3].any()) and not bool(got[5][-3:].any())     # zeros, not NaN and not the allocation's bytes


# ---- C. row strides, mask forms, alignment: the bits of the contiguous call on all three entry points


def _stride_case(form):
    H = 6
    if form == "encoder":
        q, k, v, att, table, offset, keep = _self_inputs(33, H, False)
        kw = dict(bias_by_delta=table, bias_offset=offset, key_mask=keep)
    else:
        q, k, v, keep = _cross(5, 37)
        kw = dict(key_mask=keep)
    d_out = torch.randn(q.shape, generator=torch.Generator().manual_seed(21)).to("cuda")
    return q, k, v, d_out, H, kw


def _three_entry_points(q, k, v, d_out, H, **kw):
    from rqhip import ops
    with torch.no_grad():
        out = ops.t5_attention(q, k, v, H, **kw)
        out_train, lse = ops.t5_attention_fwd_train(q, k, v, H, **kw)
        grads = ops.t5_attention_bwd(q, k, v, out_train, lse, d_out, H, **kw)
    return (out, out_train, lse) + tuple(x for x in grads if x is not None)


def _all_same_bits(got, want):
    assert len(got) == len(want)
    for x, y in zip(got, want):
        assert same_bits(x, y)


def _half_of(x, other):
    """x as the right-hand column slice of a buffer twice as wide."""
    view = torch.cat([other, x], dim=-1)[..., other.shape[-1]:]
    assert not view.is_contiguous() and view.data_ptr() % 16 == 0
    return view


@pytest.mark.parametrize("form", ["encoder", "cross"])
def test_gap9_column_slices_are_read_in_place(form, monkeypatch):
    q, k, v, d_out, H, kw = _stride_case(form)
    want = _three_entry_points(q, k, v, d_out, H, **kw)
    inner = H * 64
    if form == "encoder":            # one [R, T, 3 * inner] buffer, as a fused q/k/v projection writes it
        qkv = torch.cat([q, k, v], dim=-1)
        qs, ks, vs = qkv[..., :inner], qkv[..., inner:2 * inner], qkv[..., 2 * inner:]
        assert qs.stride(1) == ks.stride(1) == vs.stride(1) == 3 * inner
    else:                            # q of one buffer, k and v of another
        qs = _half_of(q, torch.full_like(q, 3.0))
        kv = torch.cat([k, v], dim=-1)
        ks, vs = kv[..., :inner], kv[..., inner:]
    ds = _half_of(d_out, torch.full_like(d_out, -2.0))
    assert ds.stride(1) == 2 * inner and not ks.is_contiguous() and not vs.is_contiguous()
    copies = []
    o_contig = torch.Tensor.contiguous

    def spy_contig(self, *a, **k_):
        if self.dtype == torch.float32 and not self.is_contiguous():
            copies.append(tuple(self.shape))
        return o_contig(self, *a, **k_)

    monkeypatch.setattr(torch.Tensor, "contiguous", spy_contig)
    got = _three_entry_points(qs, ks, vs, ds, H, **kw)
    monkeypatch.setattr(torch.Tensor, "contiguous", o_contig)
    assert not copies, copies
    _all_same_bits(got, want)


@pytest.mark.parametrize("form", ["encoder", "cross"])
def test_gap9_k_and_v_of_different_row_strides_are_copied(form):
    q, k, v, d_out, H, kw = _stride_case(form)
    want = _three_entry_points(q, k, v, d_out, H, **kw)
    ks = _half_of(k, torch.full_like(k, 5.0))
    vs = _half_of(v, torch.full_like(torch.cat([v, v], dim=-1), 5.0))
    assert ks.stride(1) == 2 * H * 64 and vs.stride(1) == 3 * H * 64
    _all_same_bits(_three_entry_points(q, ks, vs, d_out, H, **kw), want)


@pytest.mark.parametrize("form", ["encoder", "cross"])
def test_gap9_uint8_and_strided_key_masks(form):
    q, k, v, d_out, H, kw = _stride_case(form)
    want = _three_entry_points(q, k, v, d_out, H, **kw)
    keep = kw.pop("key_mask")
    _all_same_bits(_three_entry_points(q, k, v, d_out, H, key_mask=keep.to(torch.uint8), **kw), want)
    wide = torch.stack([keep, ~keep], dim=-1).reshape(keep.shape[0], -1)     # [Rk, 2 * Tk]: keep in the even columns
    strided = wide[:, ::2]
    assert strided.dtype == torch.bool and not strided.is_contiguous() and torch.equal(strided, keep)
    _all_same_bits(_three_entry_points(q, k, v, d_out, H, key_mask=strided, **kw), want)


@pytest.mark.parametrize("form", ["encoder", "cross"])
def test_gap9_q_off_a_16_byte_boundary_is_copied(form):
    """ops._token_rows used to hand a CONTIGUOUS view off the boundary on as it was (contiguous() returns it unchanged),
    and the library refused the call; a column slice off the boundary was always copied."""
    q, k, v, d_out, H, kw = _stride_case(form)
    want = _three_entry_points(q, k, v, d_out, H, **kw)
    base = torch.empty(q.numel() + 4, device="cuda")
    base[1:1 + q.numel()].view(q.shape).copy_(q)
    q_off = base[1:1 + q.numel()].view(q.shape)            # contiguous, one float past the boundary
    assert q_off.is_contiguous() and q_off.data_ptr() % 16 == 4 and torch.equal(q_off, q)
    _all_same_bits(_three_entry_points(q_off, k, v, d_out, H, **kw), want)
    q_col = torch.cat([torch.zeros_like(q[..., :1]), q, torch.zeros_like(q[..., :3])], dim=-1)[..., 1:1 + q.shape[-1]]
    assert q_col.stride(1) % 4 == 0 and q_col.data_ptr() % 16 == 4 and torch.equal(q_col, q)   # a slice off the boundary
    _all_same_bits(_three_entry_points(q_col, k, v, d_out, H, **kw), want)
