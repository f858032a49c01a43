"""The fused semantic-id input embedding on the GPU: ops.sid_embed_fwd / ops.sid_embed_bwd, autograd.SidEmbedFunction
(csrc/sid_embed.hip) and embed_impl = "hip" on the retrieval model (modules/model.py).

Op level.  The reference is the operator chain of modules/model.py itself (_strip_dedup_col,
_add_repeating_offset_to_rows, the embedding, _inject_sep_token_between_sids, the user / BOS concatenation) on the same
device tensors.  The forward is a gather: x must have the chain's bits and mask_out its truth values.  The backward is
gated per tensor, e = max|a - a64| / max|a64| and e_kernel <= max(8 e_torch, 2^-22) (retrieval_cases.gate; factor and
floor are those of the embedding weight gradient in tests/test_gpu_t5_attention_backward.py), e_torch from the chain's
own fp32 gradients on the device and a64 from the same chain in fp64 on the host; a destination row no token reads must
be exactly zero, and two runs must give the same bits.  The shapes are the smallest at which each mechanism can go
wrong: both column strides and mask types, every optional position, one and several scan chunks, chunks that are full,
a row that collects all padding, the narrowest and the widest row.

Model level.  small_model (d_model 64, 2 heads, d_ff 128, 2 layers, K = 16, L = 3, batch 3 with a padded item) in eval
mode: the loss and every gradient the embedding does not produce must have the operators' bits; the table, separator,
BOS and user-table gradients pass the gate against the fp64 model."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from retrieval_cases import gate, impls, loss_and_grads, reference, same_bits, small_model, synthetic_batch, to_device

pytestmark = pytest.mark.gpu

SMALL = (11, 128, True)         # the set-up of tests/test_gpu_t5_norm_impl.py

# name: B, items, L, K, d, pad, sep, prefix (None, "user", "bos"), ld_item - L, mask (None, "bool", "int64")
CASES = {
    "small": (3, 2, 3, 16, 64, "row1", True, None, 1, "bool"),
    "stripped_int64_mask": (3, 2, 3, 16, 64, "row1", True, None, 0, "int64"),
    "no_sep": (3, 2, 3, 16, 64, "row1", False, None, 1, "bool"),
    "user_prefix": (3, 2, 3, 16, 64, "row1", True, "user", 1, "bool"),
    "bos_decoder_form": (3, 1, 3, 16, 64, "none", False, "bos", 1, None),
    "d4": (3, 2, 3, 16, 4, "row1", True, None, 1, "bool"),
    "d1024": (2, 1, 3, 16, 1024, "none", True, None, 1, "bool"),
    "one_row": (1, 2, 3, 16, 64, "none", True, "user", 1, "bool"),
    "one_level": (3, 2, 1, 16, 64, "row1", True, None, 1, "bool"),
    "full_chunks": (9, 64, 2, 1, 64, "none", True, None, 1, "bool"),        # 576 matches per row, every chunk full
    "padding_row0": (9, 20, 3, 256, 128, "b_mod_items", True, "user", 1, "bool"),   # 540 tokens, row 0 hot
    # 1250 tokens that all read row 0, and as many separators: the first chunk's list is full to its last slot
    "every_token_one_row": (5, 250, 1, 1, 8, "none", True, None, 1, "bool"),
}
USER_ROWS = 7


def _model_class():
    from modules.model import EncoderDecoderRetrievalModel
    return EncoderDecoderRetrievalModel


def chain(ids, mask, table, sep, prefix_table, prefix_idx, L, ld_item, K):
    """modules/model.py's operators -> (inputs_embeds, keep-mask), in the dtype and on the device of `table`."""
    from modules.model import _strip_dedup_col
    M = _model_class()
    if mask is None:
        mask = torch.ones_like(ids)
    if ld_item != L:
        ids, mask = _strip_dedup_col(ids, ld_item, L), _strip_dedup_col(mask.long(), ld_item, L)
    mask = mask.long()
    x = F.embedding(M._add_repeating_offset_to_rows(None, ids, K, L, mask), table)
    if sep is not None:
        x, mask = M._inject_sep_token_between_sids(None, x, mask, sep, L)
    if prefix_table is not None:
        if prefix_idx is not None:
            row = F.embedding(torch.remainder(prefix_idx[:, 0], prefix_table.shape[0]), prefix_table).unsqueeze(1)
        else:
            row = prefix_table.unsqueeze(0).expand(ids.shape[0], 1, -1)
        x = torch.cat([row, x], dim=1)
        mask = torch.cat([torch.ones(mask.size(0), 1, device=mask.device), mask], dim=1)
    return x, mask


def chain_grads(inputs, params, d_x, L, ld_item, K, dtype, device):
    """The chain's (x, mask, gradients of `params` for the upstream gradient d_x), computed in dtype on device."""
    ids, mask, prefix_idx = (None if t is None else t.to(device) for t in inputs)
    leaves = [None if p is None else p.detach().to(device=device, dtype=dtype).requires_grad_(True) for p in params]
    x, keep = chain(ids, mask, leaves[0], leaves[1], leaves[2], prefix_idx, L, ld_item, K)
    x.backward(d_x.to(device=device, dtype=dtype))
    return x.detach(), keep, [None if p is None else p.grad for p in leaves]


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of one case and the chain's results, computed once: fp32 on the device, fp64 on the host."""
    from modules.model import _strip_dedup_col
    B, items, L, K, d, pad, with_sep, prefix, extra, mask_kind = CASES[name]
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    corpus = torch.randint(0, K, (200, L), generator=g)
    batch = synthetic_batch(corpus, B, items, g, pad=pad if B > 1 else "none")
    ids, mask = batch.sem_ids, batch.seq_mask
    ld_item = L + extra
    if not extra:
        ids, mask = _strip_dedup_col(ids, L + 1, L), _strip_dedup_col(mask, L + 1, L)
    mask = {None: None, "bool": mask, "int64": None if mask is None else mask.long()}[mask_kind]
    table = torch.randn(L * K, d, generator=g)
    sep = torch.randn(1, d, generator=g) if with_sep else None
    prefix_table = {None: None, "user": torch.randn(USER_ROWS, d, generator=g), "bos": torch.randn(1, d, generator=g)}[prefix]
    prefix_idx = batch.user_ids if prefix == "user" else None           # up to 99: the remainder matters
    T = (prefix is not None) + items * (L + with_sep)
    d_x = torch.randn(B, T, d, generator=g)
    inputs, params = (ids, mask, prefix_idx), (table, sep, prefix_table)
    x32, keep32, grads32 = chain_grads(inputs, params, d_x, L, ld_item, K, torch.float32, dev)
    _, _, grads64 = chain_grads(inputs, params, d_x, L, ld_item, K, torch.float64, torch.device("cpu"))
    on = lambda t: None if t is None else t.to(dev)
    return dict(L=L, K=K, ld_item=ld_item, ids=on(ids), mask=on(mask), table=on(table), sep=on(sep),
                prefix_table=on(prefix_table), prefix_idx=on(prefix_idx), d_x=on(d_x), x=x32, keep=keep32,
                grads32=grads32, grads64=grads64)


def run_fwd(c, **kw):
    from rqhip import ops
    return ops.sid_embed_fwd(c["ids"], c["mask"], c["table"], c["L"], c["ld_item"], c["sep"], c["prefix_table"],
                             c["prefix_idx"], **kw)


def run_bwd(c, **kw):
    from rqhip import ops
    rows = 0 if c["prefix_table"] is None else c["prefix_table"].shape[0]
    return ops.sid_embed_bwd(c["d_x"], c["ids"], c["mask"], c["L"], c["ld_item"], c["K"], has_sep=c["sep"] is not None,
                             prefix_rows=rows, prefix_idx=c["prefix_idx"], **kw)


@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_has_the_operators_bits(name):
    c = case(name)
    x, keep = run_fwd(c)
    assert x.dtype == torch.float32 and same_bits(x, c["x"])
    assert keep.dtype == torch.bool and torch.equal(keep, c["keep"].bool())
    x2, none = run_fwd(c, need_mask=False)
    assert none is None and same_bits(x2, x)


@pytest.mark.parametrize("name", sorted(CASES))
def test_backward_against_fp64(name):
    c = case(name)
    got = run_bwd(c)
    for what, a, a32, a64 in zip(("d_table", "d_sep", "d_prefix"), got, c["grads32"], c["grads64"]):
        if a64 is None:
            assert a is None, what
            continue
        assert a.shape == a32.shape or a.shape == a32.shape[1:], what           # d_sep is [d], the parameter [1, d]
        a = a.view(a32.shape)
        gate(f"{name} {what}", a, a32, a64, 8)
        untouched = ~a64.abs().sum(dim=-1).bool()                  # rows no token reads
        assert not bool(a[untouched.to(a.device)].any()), what
    again = run_bwd(c)
    for a, b in zip(got, again):
        assert (a is None and b is None) or same_bits(a, b)
    only_table = run_bwd(c, need_sep=False, need_prefix=False)
    assert only_table[1] is None and only_table[2] is None and same_bits(only_table[0], got[0])


def test_an_id_outside_the_table_is_clamped_forward_and_dropped_backward():
    c = dict(case("small"))
    L, K, ld = c["L"], c["K"], c["ld_item"]
    b, i = 2, 1                                           # an unpadded item (only row 1 is padded)
    ids = c["ids"].clone()
    assert bool(c["mask"][b, i * ld + L - 1])
    ids[b, i * ld + L - 1] = K                            # index (L - 1) * K + K = V
    t = i * (L + 1) + L - 1
    c["ids"] = ids
    x, keep = run_fwd(c)
    torch.cuda.synchronize()                              # returned without a fault
    others = torch.ones(x.shape[:2], dtype=torch.bool, device=x.device)
    others[b, t] = False
    assert same_bits(x[others], c["x"][others]) and torch.equal(keep, c["keep"].bool())
    assert same_bits(x[b, t], c["table"][L * K - 1])
    # the reference with that token removed: a valid id in its place and no upstream gradient at its position
    d_x = c["d_x"].clone()
    d_x[b, t] = 0
    inputs, params = (c["ids"].clone(), c["mask"], None), (c["table"], c["sep"], None)
    inputs[0][b, i * ld + L - 1] = 0
    _, _, g32 = chain_grads(inputs, params, d_x, L, ld, K, torch.float32, x.device)
    _, _, g64 = chain_grads(inputs, params, d_x, L, ld, K, torch.float64, torch.device("cpu"))
    d_table, d_sep, _ = run_bwd(c)
    gate("bad id d_table", d_table, g32[0], g64[0], 8)
    gate("bad id d_sep", d_sep.view(1, -1), g32[1], g64[1], 8)
    untouched = ~g64[0].abs().sum(dim=-1).bool()
    assert not bool(d_table[untouched.to(d_table.device)].any())


def test_autograd_function_and_needed_gradients():
    from rqhip.autograd import SidEmbedFunction
    c = case("user_prefix")
    leaves = [c[n].detach().clone().requires_grad_(n != "sep") for n in ("table", "sep", "prefix_table")]
    x, keep = SidEmbedFunction.apply(c["ids"], c["mask"], leaves[0], leaves[1], leaves[2], c["prefix_idx"], c["L"],
                                     c["ld_item"], True)
    assert x.requires_grad and not keep.requires_grad and same_bits(x.detach(), c["x"])
    x.backward(c["d_x"])
    want = run_bwd(c)
    assert leaves[1].grad is None                                        # not asked for
    assert same_bits(leaves[0].grad, want[0]) and same_bits(leaves[2].grad, want[2])


# ---- the option on the model

EMBED_GRADS = ("item_sid_embedding_table.weight", "sep_token", "bos_token", "user_embedding.weight")


def _count(monkeypatch):
    import modules.model as mm
    calls = {"fwd": 0, "bwd": 0}
    o_f, o_b = mm.ops.sid_embed_fwd, mm.ops.sid_embed_bwd

    def fwd(*a, **kw):
        calls["fwd"] += 1
        return o_f(*a, **kw)

    def bwd(*a, **kw):
        calls["bwd"] += 1
        return o_b(*a, **kw)

    monkeypatch.setattr(mm.ops, "sid_embed_fwd", fwd)
    monkeypatch.setattr(mm.ops, "sid_embed_bwd", bwd)
    return calls


@functools.lru_cache(maxsize=None)
def user_model():
    """small_model's shape with a user table of 7 rows: (fp32 model on the device, batch on the device, the fp64
    copy's loss and gradients)."""
    B, items, L, K = 3, 2, 3, 16
    g = torch.Generator().manual_seed(5)
    torch.manual_seed(5)
    corpus = torch.randint(0, K, (200, L), generator=g)
    model = _model_class()(corpus, L, K, t5_d_model=64, t5_num_heads=2, t5_d_ff=128, t5_num_layers=2,
                           num_user_bins=USER_ROWS)
    batch = synthetic_batch(corpus, B, items, g, pad="row1")
    ref = loss_and_grads(copy.deepcopy(model).double().eval(), batch)
    return model.to("cuda").eval(), to_device(batch, "cuda"), ref


def _check_model(model, batch, loss64, grads64):
    with impls(model):
        loss32, grads32 = loss_and_grads(model, batch)
    with impls(model):
        model.embed_impl = "hip"
        try:
            loss, grads = loss_and_grads(model, batch)
        finally:
            model.embed_impl = "torch"
    assert same_bits(loss, loss32)
    assert sorted(grads) == sorted(grads32) == sorted(grads64) and len(grads) > 40
    for n in sorted(grads):
        if n in EMBED_GRADS:
            gate(f"grad {n}", grads[n], grads32[n], grads64[n], 8)
        else:
            assert same_bits(grads[n], grads32[n]), n
    return [n for n in grads if n in EMBED_GRADS]


def test_model_loss_bits_and_gradients():
    model, _, batch, _ = small_model(*SMALL)
    gated = _check_model(model.eval(), batch, *reference(*SMALL))
    assert sorted(gated) == ["bos_token", "item_sid_embedding_table.weight", "sep_token"]


def test_model_with_user_bins():
    model, batch, ref = user_model()
    gated = _check_model(model, batch, *ref)
    assert sorted(gated) == sorted(EMBED_GRADS)


def test_model_with_all_five_options():
    model, _, batch, _ = small_model(*SMALL)
    _, grads64 = reference(*SMALL)
    name = "item_sid_embedding_table.weight"
    with impls(model.eval(), attention="hip_train", norm="hip", ffn="hip", head="hip"):
        _, grads32 = loss_and_grads(model, batch)
        model.embed_impl = "hip"
        try:
            loss, grads = loss_and_grads(model, batch)
        finally:
            model.embed_impl = "torch"
    assert torch.isfinite(loss)
    gate(f"all hip: grad {name}", grads[name], grads32[name], grads64[name], 8)


def test_the_path_is_taken(monkeypatch):
    model, _, batch, _ = small_model(*SMALL)
    calls = _count(monkeypatch)
    with impls(model.eval()):
        loss_and_grads(model, batch)
        with torch.no_grad():
            model(batch)
        assert calls == {"fwd": 0, "bwd": 0}                    # "torch": the fused op is never called
        model.embed_impl = "hip"
        try:
            out = model(batch)
            assert calls == {"fwd": 2, "bwd": 0}                # the encoder's front and the decoder's
            out.loss.backward()
            assert calls == {"fwd": 2, "bwd": 2}
            with torch.no_grad():
                quiet = model(batch)
            assert calls == {"fwd": 4, "bwd": 2}
            assert not quiet.loss.requires_grad and same_bits(quiet.loss, out.loss.detach())
        finally:
            model.embed_impl = "torch"


def test_generate_takes_the_path_and_keeps_its_results(monkeypatch):
    model, _, batch, _ = small_model(*SMALL)
    calls = _count(monkeypatch)
    with impls(model.eval()):
        torch.manual_seed(1)
        want = model.generate_next_sem_id(batch)
        assert calls["fwd"] == 0
        model.embed_impl = "hip"
        try:
            torch.manual_seed(1)
            got = model.generate_next_sem_id(batch)
        finally:
            model.embed_impl = "torch"
        assert calls == {"fwd": 1, "bwd": 0}                    # the encoder's front; the per-step lookups stay
    assert torch.equal(got.sem_ids, want.sem_ids) and same_bits(got.log_probas, want.log_probas)
