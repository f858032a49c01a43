"""The fused T5 attention (csrc/t5_attention.hip, ops.t5_attention, the `attention_impl` switch) on the host: argument
checks of the C entry point, its support table, the relative-position bias as a table by j - i, the ancestor table of
the incremental decoder against an index_select + cat cache, and the switch's default and fall-backs.  No GPU needed."""
import pytest
import torch

from retrieval_cases import tiny_batch, tiny_model


def _att(l, *, q=0, R=4, Rk=4, H=6, d_kv=64, Tq=8, Tk=8, ld=None, anc=None, past=0, bias=None, n_delta=0, offset=0):
    ld = H * 64 if ld is None else ld
    # q, k, v and out stay null: they are checked last, so a case that passed every other check still launches nothing
    return l.rqhip_t5_attention(None, ld, None, None, ld, R, Rk, H, d_kv, Tq, Tk, bias, n_delta, offset, None, 0, past,
                                anc, 4, R, None, ld, None)


def test_t5_attention_argument_checks_without_gpu():
    from rqhip import _lib
    l = _lib.lib()
    assert _att(l, d_kv=32) == -2 and b"d_kv" in l.rqhip_last_error()
    assert _att(l, d_kv=128) == -2
    assert _att(l, Tk=257) == -2 and b"<= 256" in l.rqhip_last_error()
    assert _att(l, Tq=257, Tk=256) == -2
    assert _att(l, R=10, Rk=4) == -1 and b"multiple" in l.rqhip_last_error()
    assert _att(l) == -1 and b"null pointer" in l.rqhip_last_error()                 # null q (and k, v, out)
    assert _att(l, bias=16, n_delta=15, offset=7) == -1 and b"null pointer" in l.rqhip_last_error()
    assert _att(l, H=0) == -1 and _att(l, Tq=0) == -1 and _att(l, past=-1) == -1
    assert _att(l, ld=6 * 64 - 4) == -1 and b"row strides" in l.rqhip_last_error()
    assert _att(l, ld=6 * 64 + 2) == -1
    # the bias table must cover every delta j - i - past of the call
    assert _att(l, bias=16, n_delta=14, offset=7) == -1 and b"bias table" in l.rqhip_last_error()
    assert _att(l, bias=16, n_delta=15, offset=6) == -1
    # the ancestor table belongs to the one-token step
    assert _att(l, anc=16, Tq=2, Tk=3, past=2) == -1 and b"ancestor" in l.rqhip_last_error()
    assert _att(l, anc=16, Tq=1, Tk=5, past=2) == -1
    assert _att(l, R=0, Rk=0) == 0                       # nothing to do


def test_t5_attention_supported_truth_table():
    from rqhip import _lib, ops
    l = _lib.lib()
    for H in (1, 6, 8, 64):
        for Tq, Tk in ((1, 1), (7, 7), (1, 256), (256, 256), (81, 101)):
            assert l.rqhip_t5_attention_supported(64, H, Tq, Tk) == 1
            assert ops.t5_attention_supported(torch.float32, 64, H, Tq, Tk)
    assert not ops.t5_attention_supported(torch.float32, 64, 6, 257, 16)
    assert not ops.t5_attention_supported(torch.float32, 64, 6, 16, 257)
    assert not ops.t5_attention_supported(torch.float32, 32, 6, 16, 16)
    assert not ops.t5_attention_supported(torch.float32, 128, 6, 16, 16)
    assert not ops.t5_attention_supported(torch.float32, 64, 0, 16, 16)
    assert not ops.t5_attention_supported(torch.float32, 64, 6, 0, 16)
    assert not ops.t5_attention_supported(torch.float16, 64, 6, 16, 16)
    assert not ops.t5_attention_supported(torch.bfloat16, 64, 6, 16, 16)
    assert not ops.t5_attention_supported(torch.float64, 64, 6, 16, 16)


def _attention(is_decoder, heads=6):
    from modules.t5 import T5Attention, T5Config
    torch.manual_seed(3)
    att = T5Attention(T5Config(64, d_model=32, num_heads=heads, is_decoder=is_decoder), has_relative_attention_bias=True)
    torch.nn.init.normal_(att.relative_attention_bias.weight)
    return att


def _bias_from_table(att, Tq, Tk, past):
    table, offset = att.delta_table(Tq, Tk, past)
    i = torch.arange(Tq)[:, None]
    j = torch.arange(Tk)[None, :]
    assert table.shape == (Tq + Tk - 1, att.n_heads)
    return table[(j - i - past) + offset].permute(2, 0, 1).unsqueeze(0)


@pytest.mark.parametrize("T", [1, 7, 81, 200, 256])
def test_delta_table_reproduces_compute_bias_encoder(T):
    att = _attention(is_decoder=False)
    with torch.no_grad():
        assert torch.equal(_bias_from_table(att, T, T, 0), att.compute_bias(T, T))


@pytest.mark.parametrize("past", [0, 1, 3])
@pytest.mark.parametrize("Tq", [1, 4])
def test_delta_table_reproduces_compute_bias_decoder(Tq, past):
    att = _attention(is_decoder=True, heads=8)
    with torch.no_grad():
        assert torch.equal(_bias_from_table(att, Tq, past + Tq, past), att.compute_bias(Tq, past + Tq, past))
        # long histories reach the logarithmic buckets
        assert torch.equal(_bias_from_table(att, 1, 201, 200), att.compute_bias(1, 201, 200))
    # the buckets are computed once per range of deltas
    key = (-(Tq - 1) - past, Tq, torch.device("cpu"))
    first = att._delta_buckets[key]
    att.delta_table(Tq, past + Tq, past)
    assert att._delta_buckets[key] is first


def test_delta_bucket_cache_is_bounded():
    from modules.t5 import MAX_DELTA_BUCKETS
    att = _attention(is_decoder=False)
    with torch.no_grad():
        for T in range(1, 3 * MAX_DELTA_BUCKETS):
            att.delta_table(T, T, 0)
            assert len(att._delta_buckets) <= MAX_DELTA_BUCKETS
        assert torch.equal(_bias_from_table(att, 9, 9, 0), att.compute_bias(9, 9))


def test_ancestor_table_reproduces_the_index_select_and_cat_cache():
    from modules.t5 import T5DecodeCache
    g = torch.Generator().manual_seed(5)
    B, k, steps, inner = 3, 4, 5, 8
    rows = B * k
    cache = T5DecodeCache(1, steps, rows, inner, "cpu")
    slab = cache.slabs[0][0]
    ref = None                                   # the operators' cache: [rows, t, inner], reordered and grown per step
    for t in range(steps):
        R = B if t == 0 else rows
        if t > 0:
            parent = torch.randint(0, ref.shape[0], (B, k), generator=g)
            ref = ref.index_select(0, parent.flatten())
            cache.reorder(parent)
        assert cache.pos == t
        fresh = torch.randn(R, inner, generator=g)
        slab[t, :R] = fresh
        ref = fresh[:, None] if ref is None else torch.cat([ref, fresh[:, None]], dim=1)
        # the kernel's addressing: key s < t of row r is row anc[r, s] of slab s, key t is row r of slab t
        anc = cache.anc[:R].long()
        got = torch.stack([slab[s, anc[:, s]] for s in range(t)] + [slab[t, :R]], dim=1)
        assert torch.equal(got, ref)
    assert cache.anc.dtype == torch.int32


def test_attention_impl_defaults_to_torch_and_is_pushed_to_both_stacks():
    m = tiny_model()
    assert m.attention_impl == "torch"
    assert m.encoder.encoder.attention_impl == "torch" and m.t5_decoder.attention_impl == "torch"
    assert "attention_impl" not in m.state_dict() and not any("delta" in n for n in m.state_dict())
    batch = tiny_batch()
    m.eval()
    want = m(batch).loss
    m.attention_impl = "hip"
    # under grad the operators run: same bits, and a graph to differentiate
    got = m(batch).loss
    assert m.encoder.encoder.attention_impl == "hip" and m.t5_decoder.attention_impl == "hip"
    assert torch.equal(got, want) and got.requires_grad
    # CPU tensors under no_grad: the operators as well
    with torch.no_grad():
        assert torch.equal(m(batch).loss, want)
    m.attention_impl = "triton"
    with pytest.raises(ValueError, match="attention_impl"):
        m(batch)


def test_hip_is_not_taken_under_grad_in_train_mode_or_on_the_host():
    from modules.t5 import T5Config, T5Stack
    stack = T5Stack(T5Config(16, d_model=8, num_heads=2, d_ff=8, num_layers=1)).eval()
    stack.attention_impl = "hip"

    class OnDevice:                # hip_attention_active reads only these
        is_cuda, dtype = True, torch.float32

    with torch.no_grad():
        assert stack.hip_attention_active(OnDevice, 7, 7)
        assert stack.hip_attention_active(OnDevice, 1, 3, 81)
        assert not stack.hip_attention_active(OnDevice, 7, 300)           # unsupported length
        assert not stack.hip_attention_active(OnDevice, 1, 3, 300)        # ... of the encoder output
        assert not stack.hip_attention_active(torch.zeros(1, 7, 8), 7, 7)  # host tensor
        stack.train()
        assert not stack.hip_attention_active(OnDevice, 7, 7)             # attention dropout is active
        stack.eval()
        stack.attention_impl = "torch"
        assert not stack.hip_attention_active(OnDevice, 7, 7)
        stack.attention_impl = "hip"
    assert not stack.hip_attention_active(OnDevice, 7, 7)                 # grad enabled
    x = torch.randn(2, 7, 8)
    with torch.no_grad():
        want = stack(x)
        with pytest.raises(ValueError, match="decode_cache"):
            stack(x[:, :1], decode_cache=stack.new_decode_cache(3, 2, "cpu"))
    stack.attention_impl = "torch"
    with torch.no_grad():
        assert torch.equal(stack(x), want)
