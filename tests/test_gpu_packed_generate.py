"""`model.encoder_rows = "packed"` in `generate`, `generate_next_sem_id` and `recommend_items` (modules/model.py), and the
`encoder_rows.mode` binding in evaluate_decoder.evaluate: the search on the valid encoder tokens only, against the padded
fused run on the same batch.

Model and batch of tests/test_gpu_packed_model.py: d_model 64, 2 heads, d_ff 96, 2 layers, K = 16, L = 3, a 200-row
corpus, batch 5 with histories of 4, 3, 2, 1 and 4 items out of 4 slots, with and without a user token (N = 61 / 56
packed tokens, bound 17 / 16), top_k_for_generation = 4.

Every row-local kernel is batch-independent by contract (include/rqhip.h), the packed encoder attention keeps the padded
bits (tests/test_gpu_t5_attention_packed.py) and so does the beams' cross-attention
(tests/test_gpu_t5_attention_packed_beams.py), so every gate is torch.equal or a call count."""
import contextlib
import functools

import pytest
import torch

from retrieval_cases import LAYERS, setting, synthetic_batch, to_device

pytestmark = pytest.mark.gpu

B, ITEMS, L, K, TOP_K = 5, 4, 3, 16, 4
COUNTS = [4, 3, 2, 1, 4]                       # pad = "b_mod_items": the last b % 4 items of row b are padding
FUSED = dict(attention="hip_train", norm="hip", ffn="hip", head="hip", embed="hip")
SETTINGS = {"fused": (FUSED, "fp32"), "proj": ({**FUSED, "proj": "hip"}, "fp32"), "bf16": ({**FUSED, "proj": "hip"}, "bf16")}
SPIED = ("t5_attention", "t5_attention_packed", "t5_attention_packed_beams", "rows_pack", "rows_unpack")
# the padded search (the calls of the commit before packed rows reached `generate`): one launch per encoder block, and
# per step and decoder block one cached self-attention and one cross-attention
PADDED_CALLS = {"t5_attention": LAYERS + 2 * LAYERS * L, "t5_attention_packed": 0, "t5_attention_packed_beams": 0,
                "rows_pack": 0, "rows_unpack": 0}


def _counted(batch, counts=None):
    from data.schemas import CountedSeqBatch
    if counts is None:
        counts = batch.seq_mask.view(batch.seq_mask.shape[0], -1, L + 1)[:, :, 0].sum(1).cpu()
    return CountedSeqBatch(*batch, item_counts=counts.to(torch.int64))


@functools.lru_cache(maxsize=None)
def _models(user):
    """(the model on the device, the counted batch, the plain one)."""
    from modules.model import EncoderDecoderRetrievalModel
    g = torch.Generator().manual_seed(31)
    torch.manual_seed(31)
    corpus = torch.randint(0, K, (200, L), generator=g)
    model = EncoderDecoderRetrievalModel(corpus, L, K, t5_d_model=64, t5_num_heads=2, t5_d_ff=96, t5_num_layers=LAYERS,
                                         num_user_bins=10 if user else None, top_k_for_generation=TOP_K)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("layer_norm.weight"):
                p.copy_(1 + 0.5 * torch.randn(p.shape, generator=g))
    plain = to_device(synthetic_batch(corpus, B, ITEMS, g, pad="b_mod_items"), "cuda")
    counted = _counted(plain)
    assert counted.item_counts.tolist() == COUNTS
    return model.cuda().eval(), counted, plain


@contextlib.contextmanager
def _rows(model, rows, arith="fp32", beam="sample"):
    model.encoder_rows, model.matmul_arith, model.beam_impl = rows, arith, beam
    try:
        yield model
    finally:
        model.encoder_rows, model.matmul_arith, model.beam_impl = "padded", "fp32", "sample"
        model._push_attention_impl()


@contextlib.contextmanager
def _spy():
    """Counts the calls of the attention ops, padded and packed, and of the pack ops; `kv_rows`: the rows of k of every
    t5_attention_packed_beams call."""
    from rqhip import ops
    calls = dict.fromkeys(SPIED, 0)
    calls["kv_rows"] = []
    with pytest.MonkeyPatch.context() as mp:
        for name in SPIED:
            def counted(*a, _name=name, _real=getattr(ops, name), **kw):
                calls[_name] += 1
                if _name == "t5_attention_packed_beams":
                    calls["kv_rows"].append(a[1].shape[0])
                return _real(*a, **kw)
            mp.setattr(ops, name, counted)
        yield calls


def _search(model, batch, seed=11):
    torch.manual_seed(seed)
    with _spy() as calls:
        out = model.generate_next_sem_id(batch)
    kv_rows = calls.pop("kv_rows")
    return out, calls, kv_rows


def _same(a, b):
    assert a.sem_ids.shape == b.sem_ids.shape == (B, TOP_K, L) and a.sem_ids.dtype == b.sem_ids.dtype == torch.int64
    assert a.log_probas.shape == b.log_probas.shape == (B, TOP_K) and a.log_probas.dtype == torch.float32
    assert torch.equal(a.sem_ids, b.sem_ids) and torch.equal(a.log_probas, b.log_probas)


@pytest.mark.parametrize("beam", ["exact", "sample"])
@pytest.mark.parametrize("name", list(SETTINGS))
@pytest.mark.parametrize("user", [False, True], ids=["no user token", "user token"])
def test_the_packed_search_returns_the_padded_bits(user, name, beam):
    model, counted, _ = _models(user)
    choices, arith = SETTINGS[name]
    N = sum(COUNTS) * (L + 1) + (B if user else 0)
    assert N == (61 if user else 56)
    with setting(model, **choices):
        with _rows(model, "padded", arith, beam):
            want, calls, _ = _search(model, counted)
            assert calls == PADDED_CALLS
            want_items = model.recommend_items(counted)
        with _rows(model, "packed", arith, beam):
            got, calls, kv_rows = _search(model, counted)
            assert calls == {"rows_pack": 1, "rows_unpack": 0, "t5_attention_packed": LAYERS,
                             "t5_attention_packed_beams": LAYERS * L, "t5_attention": LAYERS * L}
            assert kv_rows == [N] * (LAYERS * L)
            torch.manual_seed(11)
            got_items = model.recommend_items(counted)
    _same(got, want)
    assert bool(torch.isfinite(want.log_probas).any())
    if beam == "exact":          # no noise: recommend_items repeats the search, whatever the seed
        _same(got_items, got)
        assert torch.equal(got_items.items, want_items.items) and torch.equal(got_items.scores, want_items.scores)
        assert got_items.items.shape == (B, TOP_K) and bool((got_items.items >= 0).any())


@pytest.mark.parametrize("beam", ["exact", "sample"])
def test_recommend_items_under_one_seed(beam):
    model, counted, _ = _models(True)
    with setting(model, **FUSED):
        recs = []
        for rows in ("padded", "packed"):
            with _rows(model, rows, beam=beam):
                torch.manual_seed(5)
                recs.append(model.recommend_items(counted, n_items=6))
    assert torch.equal(recs[0].items, recs[1].items) and torch.equal(recs[0].scores, recs[1].scores)
    assert torch.equal(recs[0].sem_ids, recs[1].sem_ids) and torch.equal(recs[0].log_probas, recs[1].log_probas)
    assert recs[0].items.shape == (B, 6)


def test_dispatch():
    model, counted, plain = _models(False)
    with setting(model, **FUSED):
        with _rows(model, "padded", beam="exact"):
            want, today, _ = _search(model, counted)
            assert today == PADDED_CALLS
        with _rows(model, "packed", beam="exact"):
            # a plain TokenizedSeqBatch: nothing says how long the rows are
            got, calls, _ = _search(model, plain)
            _same(got, want)
            assert calls == today
            # generate itself, with and without the counts
            from modules.model import _strip_dedup_col
            ids = _strip_dedup_col(plain.sem_ids, L + 1, L)
            mask = _strip_dedup_col(plain.seq_mask.long(), L + 1, L)
            with _spy() as calls:
                a = model.generate(mask, ids, plain.user_ids)
                assert calls["rows_pack"] == 0
                b = model.generate(mask, ids, plain.user_ids, item_counts=counted.item_counts)
                assert calls["rows_pack"] == 1 and calls["t5_attention_packed_beams"] == LAYERS * L
            assert torch.equal(a[0], want.sem_ids) and torch.equal(b[0], want.sem_ids) and torch.equal(b[1], want.log_probas)
            # a row without a token (count 0, no user token) would change meaning: the padded path
            empty = plain._replace(sem_ids=plain.sem_ids.clone(), seq_mask=plain.seq_mask.clone())
            empty.sem_ids[2], empty.seq_mask[2] = -1, False
            assert _counted(empty).item_counts.tolist() == [4, 3, 0, 1, 4]
            got, calls, _ = _search(model, _counted(empty))
            assert calls == today
        with _rows(model, "padded", beam="exact"):
            want_empty, _, _ = _search(model, empty)
        _same(got, want_empty)
        with _rows(model, "packed", beam="exact"):
            with pytest.raises(ValueError, match="item_counts"):
                model.generate_next_sem_id(_counted(plain, torch.tensor([1, 2])))
    # attention_impl = "torch": the operators, no fused attention at all
    with setting(model, **{**FUSED, "attention": "torch"}):
        with _rows(model, "padded", beam="exact"):
            want_torch, calls, _ = _search(model, counted)
            assert all(v == 0 for v in calls.values())
        with _rows(model, "packed", beam="exact"):
            got, calls, _ = _search(model, counted)
            assert all(v == 0 for v in calls.values())
        _same(got, want_torch)
    # with a user token a row without items still has one token: packed
    model_u, _, plain_u = _models(True)
    empty = plain_u._replace(sem_ids=plain_u.sem_ids.clone(), seq_mask=plain_u.seq_mask.clone())
    empty.sem_ids[2], empty.seq_mask[2] = -1, False
    with setting(model_u, **FUSED):
        with _rows(model_u, "padded", beam="exact"):
            want, _, _ = _search(model_u, empty)
        with _rows(model_u, "packed", beam="exact"):
            got, calls, kv_rows = _search(model_u, _counted(empty))
            assert calls["rows_pack"] == 1 and kv_rows == [61 - 2 * (L + 1)] * (LAYERS * L)
        _same(got, want)
        model_u.encoder_rows = "ragged"
        try:
            with pytest.raises(ValueError, match="encoder_rows"):
                model_u.generate_next_sem_id(_counted(plain_u))
        finally:
            model_u.encoder_rows = "padded"


def test_the_decode_step_s_stack_checks():
    """What still cannot go with packed encoder rows raises in the stack (modules/t5.py)."""
    from modules.t5 import PackedRows
    model, counted, _ = _models(False)
    dec = model.t5_decoder
    N, d = 56, 64
    cu = torch.zeros(B + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(torch.tensor(COUNTS) * (L + 1), 0)
    rows = PackedRows(cu.cuda(), 16, B, N)
    enc = torch.randn(1, N, d, device="cuda")
    x = torch.randn(B * TOP_K, 1, d, device="cuda")
    with setting(model, **FUSED):
        with torch.no_grad():
            kv = dec.cross_kv(enc)
            slabs = dec.new_decode_cache(L, B * TOP_K, "cuda")
            out = dec(x, cross_kv=kv, decode_cache=slabs, encoder_packed=rows)           # accepted together
            assert out.shape == x.shape and bool(torch.isfinite(out).all())
            with pytest.raises(ValueError, match="mask"):
                dec(x, cross_kv=kv, decode_cache=slabs, encoder_packed=rows,
                    encoder_attention_mask=torch.ones(B, 16, device="cuda"))
            past = [(torch.zeros(B * TOP_K, 2, 1, 64, device="cuda"),) * 2] * LAYERS
            with pytest.raises(ValueError, match="past_key_values"):
                dec(x, cross_kv=kv, past_key_values=past, encoder_packed=rows)
            with pytest.raises(ValueError, match="multiple"):
                dec(x[:7], cross_kv=kv, decode_cache=slabs, encoder_packed=rows)
        with pytest.raises(ValueError, match="beams"):                                    # grad enabled, beams > 1
            dec(x, cross_kv=kv, encoder_packed=rows)


def test_evaluate_with_the_packed_binding(tmp_path):
    """evaluate_decoder.evaluate reads `encoder_rows.mode`: the metrics of the padded run, from packed searches."""
    import evaluate_decoder
    import train_decoder
    from data.processed import RecDataset
    from modules.tokenizer.semids import SemanticIdTokenizer
    root = str(tmp_path) + "/"
    shared = dict(dataset_folder="synthetic:300", dataset=RecDataset.AMAZON, batch_size=16, vae_input_dim=768,
                  vae_hidden_dims=[32], vae_embed_dim=16, vae_codebook_size=16, vae_n_layers=3, vae_n_cat_feats=0, t5_d_model=64,
                  t5_num_heads=2, t5_d_ff=128, t5_num_layers=2, top_k_for_generation=10, top_k_eval_list=[1, 5, 10],
                  pretrained_rqvae_path=root + "rqvae.pt")
    torch.manual_seed(0)
    tok = SemanticIdTokenizer(input_dim=768, hidden_dims=[32], output_dim=16, codebook_size=16, n_layers=3, n_cat_feats=0)
    torch.save({"iter": 0, "model": tok.rq_vae.state_dict()}, root + "rqvae.pt")
    gin = train_decoder.gin
    gin.clear_config()
    try:
        torch.manual_seed(0)
        checkpoint = train_decoder.train(**shared, iterations=1, partial_eval_every=100, full_eval_every=100, log_every=1,
                                         learning_rate=0.001, weight_decay=0.0001, max_grad_norm=1.0,
                                         save_dir_root=root)["checkpoint"]
        with _spy() as calls:
            want = evaluate_decoder.evaluate(**shared, checkpoint_path=checkpoint, beam_impl="exact", max_batches=2)
        assert calls["rows_pack"] == calls["t5_attention_packed_beams"] == 0
        gin.parse_config('encoder_rows.mode = "packed"')
        with _spy() as calls:
            got = evaluate_decoder.evaluate(**shared, checkpoint_path=checkpoint, beam_impl="exact", max_batches=2)
        assert calls["rows_pack"] == 2 and calls["t5_attention_packed_beams"] == 2 * 2 * 3
    finally:
        gin.clear_config()
    assert got == want and got["users"] == 32 and set(got) == {"ndcg", "users", "h@1", "h@5", "h@10"}
