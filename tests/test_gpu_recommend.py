"""model.recommend_items and recommend.recommend: the items the retrieval model names, against the Python oracle of
tests/sid_items_cases.py applied to the model's own beams, under the exact search (two calls give the same beams).

The model is retrieval_cases' tiny model with the hand-made 40-row corpus of sid_items_cases as its `codebooks`: six
tuples, one of them shared by 30 items.  The batch's histories and targets are corpus items with their real dedup ranks.
The end-to-end test trains for a few steps on `synthetic:300`, as test_gpu_evaluate_decoder.py does."""
import functools
import inspect
import random

import pytest
import torch

import sid_items_cases as cases
from retrieval_cases import tiny_model

pytestmark = pytest.mark.gpu

L = 3
USERS, T = 6, 4


def _batch(rows, seed):
    """USERS users with T history items each (user u's last u % T items padded) and a target, all corpus items."""
    from data.schemas import TokenizedSeqBatch
    rnd = random.Random(seed)
    ranks = cases.dedup_ranks(rows)
    cached = [list(row) + [r] for row, r in zip(rows, ranks)]
    hist, fut = [], []
    for u in range(USERS):
        seen = [cached[rnd.randrange(len(rows))] for _ in range(T)]
        if u == 2:
            seen[1] = seen[0]                            # the same item twice
        for j in range(T - u % T, T):
            seen[j] = [-1] * (L + 1)
        hist.append([v for item in seen for v in item])
        fut.append(cached[rnd.randrange(len(rows))])
    fut[1] = hist[1][: L + 1]                            # user 1's target is one of their own history items
    sem_ids = torch.tensor(hist)
    return TokenizedSeqBatch(torch.zeros(USERS, 1, dtype=torch.long), sem_ids, torch.tensor(fut), sem_ids >= 0, None, None)


def _model(rows):
    model = tiny_model()
    model.codebooks = torch.tensor(rows, dtype=torch.int64)
    model = model.cuda().eval()
    model.beam_impl = "exact"
    return model


@functools.lru_cache(maxsize=None)
def _colliding():
    from retrieval_cases import to_device
    rows = cases.hand_corpus()
    return _model(rows), to_device(_batch(rows, 3), "cuda"), rows


def _oracle(rows, out, n, history):
    items, scores = cases.topn(rows, out.sem_ids.tolist(), out.log_probas.tolist(), n,
                               None if history is None else history.tolist())
    return torch.tensor(items, device="cuda"), torch.tensor(scores, dtype=torch.float32, device="cuda")


@pytest.mark.parametrize("attention", ["torch", "hip"])
def test_recommend_items_is_generate_plus_the_oracles_expansion(attention):
    model, batch, rows = _colliding()
    model.attention_impl = attention
    try:
        ref = model.generate_next_sem_id(batch)
        for exclude in (True, False):
            for n in (None, 40):
                rec = model.recommend_items(batch, n_items=n, exclude_history=exclude)
                assert torch.equal(rec.sem_ids, ref.sem_ids) and torch.equal(rec.log_probas, ref.log_probas)
                n_out = model.top_k_for_generation if n is None else n
                assert rec.items.shape == (USERS, n_out) and rec.scores.shape == (USERS, n_out)
                want_items, want_scores = _oracle(rows, ref, n_out, batch.sem_ids if exclude else None)
                assert torch.equal(rec.items, want_items) and torch.equal(rec.scores, want_scores)
    finally:
        model.attention_impl = "torch"
    # the search found something to expand: all six tuples are finite beams of every user
    assert int(torch.isfinite(ref.log_probas).sum(dim=1).min()) == 6


def test_no_history_item_is_recommended_and_an_item_hit_implies_an_earlier_tuple_hit():
    from rqhip import ops
    model, batch, rows = _colliding()
    n = 40                                               # every corpus item fits: each target is found without exclusion
    rec = model.recommend_items(batch, n_items=n, exclude_history=True)
    history = batch.sem_ids.reshape(USERS, T, L + 1).tolist()
    for u in range(USERS):
        seen = {i for i in cases.items_of(rows, history[u]) if i >= 0}
        assert seen and not seen & set(rec.items[u].tolist()), u
        assert len([i for i in rec.items[u].tolist() if i >= 0]) == 40 - len(seen)
    # user 1's target is in their history, so with the exclusion it cannot be hit
    target_item = model._item_index_for_codebooks().items_of(batch.sem_ids_fut)
    assert target_item.tolist() == cases.items_of(rows, batch.sem_ids_fut.tolist()) and int(target_item.min()) >= 0
    assert int(target_item[1]) not in rec.items[1].tolist()
    rec = model.recommend_items(batch, n_items=n, exclude_history=False)
    item_pos = ops.topk_first_match(target_item[:, None].contiguous(), rec.items[:, :, None].contiguous())
    tuple_pos = ops.topk_first_match(batch.sem_ids_fut[:, :L].contiguous(), rec.sem_ids)
    assert bool((item_pos >= 0).all())
    assert bool((tuple_pos >= 0).all()) and bool((tuple_pos <= item_pos).all())


def test_collision_free_corpus_gives_the_beams_own_items():
    from retrieval_cases import to_device
    from rqhip import ops
    rows = [[i % 4, i // 4, (i * 5) % 16] for i in range(12)]          # 12 distinct rows
    assert len({tuple(r) for r in rows}) == 12
    model = _model(rows)
    batch = to_device(_batch(rows, 4), "cuda")
    names = list(model.state_dict())
    k = model.top_k_for_generation
    rec = model.recommend_items(batch, n_items=k, exclude_history=False)
    assert list(model.state_dict()) == names
    number = {tuple(r): i for i, r in enumerate(rows)}
    finite = torch.isfinite(rec.log_probas)
    assert int(finite.sum(dim=1).min()) >= 4
    for u in range(USERS):
        own = [number[tuple(b)] for b, ok in zip(rec.sem_ids[u].tolist(), finite[u].tolist()) if ok]
        assert rec.items[u].tolist() == own + [-1] * (k - len(own))
    assert torch.equal(rec.scores, rec.log_probas)
    # item-level and tuple-level ranks agree (a -inf beam names no item: its ids are taken out of the tuple match)
    target_item = model._item_index_for_codebooks().items_of(batch.sem_ids_fut)
    live_ids = torch.where(finite[:, :, None], rec.sem_ids, torch.full_like(rec.sem_ids, -1))
    item_pos = ops.topk_first_match(target_item[:, None].contiguous(), rec.items[:, :, None].contiguous())
    tuple_pos = ops.topk_first_match(batch.sem_ids_fut[:, :L].contiguous(), live_ids)
    assert torch.equal(item_pos, tuple_pos) and bool((item_pos >= 0).any())


# ---- end to end: train a few steps, then recommend

KS = [1, 5, 10]


def _config(**over):
    """The small config of test_gpu_evaluate_decoder.py."""
    from data.processed import RecDataset
    cfg = dict(dataset_folder="synthetic:300", dataset=RecDataset.AMAZON, batch_size=16, iterations=8, partial_eval_every=4,
               full_eval_every=8, log_every=1, learning_rate=0.001, weight_decay=0.0001, max_grad_norm=1.0,
               vae_input_dim=768, vae_hidden_dims=[32], vae_embed_dim=16, vae_codebook_size=16, vae_n_layers=3,
               vae_n_cat_feats=0, t5_d_model=64, t5_num_heads=2, t5_d_ff=128, t5_num_layers=2, top_k_for_generation=10,
               top_k_eval_list=KS)
    cfg.update(over)
    return cfg


def _only(fn, cfg, **over):
    params = inspect.signature(fn).parameters
    return dict({k: v for k, v in cfg.items() if k in params and k not in ("attention_impl",)}, **over)


def test_recommend_end_to_end(tmp_path):
    import evaluate_decoder
    import recommend
    import train_decoder
    from modules.tokenizer.semids import SemanticIdTokenizer
    root = str(tmp_path) + "/"
    cfg = _config(save_dir_root=root)
    torch.manual_seed(0)
    tok = SemanticIdTokenizer(input_dim=cfg["vae_input_dim"], hidden_dims=cfg["vae_hidden_dims"],
                              output_dim=cfg["vae_embed_dim"], codebook_size=cfg["vae_codebook_size"],
                              n_layers=cfg["vae_n_layers"], n_cat_feats=cfg["vae_n_cat_feats"])
    torch.save({"iter": 0, "model": tok.rq_vae.state_dict()}, root + "rqvae.pt")
    cfg["pretrained_rqvae_path"] = root + "rqvae.pt"
    torch.manual_seed(0)
    checkpoint = train_decoder.train(**cfg)["checkpoint"]

    sid = evaluate_decoder.evaluate(**_only(evaluate_decoder.evaluate, cfg, checkpoint_path=checkpoint, beam_impl="exact"))
    n_items = 12
    results = []
    for seed in (1, 2):
        torch.manual_seed(seed)
        results.append(recommend.recommend(**_only(recommend.recommend, cfg, checkpoint_path=checkpoint, beam_impl="exact",
                                                   n_items=n_items, exclude_history=False,
                                                   output_path=root + f"items_{seed}.pt")))
    assert results[0] == results[1]
    res = results[0]
    assert set(res) == {"item", "sid", "users", "targets_in_history"}
    assert res["users"] == 150 == sid["users"]
    assert res["sid"] == {name: v for name, v in sid.items() if name != "users"}
    assert set(res["item"]) == set(res["sid"]) == {"ndcg"} | {f"h@{k}" for k in KS}
    for k in KS:
        print(f"h@{k}: item {res['item'][f'h@{k}']:.4f} tuple {res['sid'][f'h@{k}']:.4f}")
        assert 0.0 <= res["item"][f"h@{k}"] <= res["sid"][f"h@{k}"] <= 1.0
    assert isinstance(res["targets_in_history"], int) and 0 <= res["targets_in_history"] <= 150
    saved = [torch.load(root + f"items_{seed}.pt") for seed in (1, 2)]
    assert saved[0]["items"].shape == (150, n_items) and saved[0]["items"].dtype == torch.int64
    assert saved[0]["scores"].shape == (150, n_items) and saved[0]["scores"].dtype == torch.float32
    assert torch.equal(saved[0]["items"], saved[1]["items"]) and torch.equal(saved[0]["scores"], saved[1]["scores"])
    # the default excludes the history: the tuple metrics and the count are the same, no history item is returned
    excl = recommend.recommend(**_only(recommend.recommend, cfg, checkpoint_path=checkpoint, max_batches=2))
    assert excl["users"] == 32 and set(excl) == set(res)
