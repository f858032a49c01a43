"""evaluate_decoder.evaluate end to end: a short train_decoder.train run on a synthetic corpus, then the metrics of its
checkpoint under the exact search (the same under every seed) and under the sampling search, and the error for a
checkpoint that was trained on another corpus.

The tokenizer of these runs has random weights, and `evaluate` is to be called under other seeds than `train`, so the
RQ-VAE's weights are saved once and both get them as pretrained_rqvae_path."""
import pytest
import torch

pytestmark = pytest.mark.gpu

KS = [1, 5, 10]
USERS = 150                     # data.processed.synthetic_sequences: max(64, 300 // 2) per split
KEYS = {"ndcg", "users"} | {f"h@{k}" for k in KS}


def _config(**over):
    """The small config of test_gpu_train_decoder.py."""
    from data.processed import RecDataset
    cfg = dict(dataset_folder="synthetic:300", dataset=RecDataset.AMAZON, batch_size=16, iterations=8, partial_eval_every=4,
               full_eval_every=8, log_every=1, learning_rate=0.001, weight_decay=0.0001, max_grad_norm=1.0,
               vae_input_dim=768, vae_hidden_dims=[32], vae_embed_dim=16, vae_codebook_size=16, vae_n_layers=3,
               vae_n_cat_feats=0, t5_d_model=64, t5_num_heads=2, t5_d_ff=128, t5_num_layers=2, top_k_for_generation=10,
               top_k_eval_list=KS)
    cfg.update(over)
    return cfg


def _eval_config(cfg, **over):
    import inspect
    import evaluate_decoder
    params = inspect.signature(evaluate_decoder.evaluate).parameters
    return dict({k: v for k, v in cfg.items() if k in params and k not in ("attention_impl",)}, **over)


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    import train_decoder
    from modules.tokenizer.semids import SemanticIdTokenizer
    root = str(tmp_path_factory.mktemp("evaluate")) + "/"
    cfg = _config(save_dir_root=root)
    torch.manual_seed(0)
    tok = SemanticIdTokenizer(input_dim=cfg["vae_input_dim"], hidden_dims=cfg["vae_hidden_dims"],
                              output_dim=cfg["vae_embed_dim"], codebook_size=cfg["vae_codebook_size"],
                              n_layers=cfg["vae_n_layers"], n_cat_feats=cfg["vae_n_cat_feats"])
    torch.save({"iter": 0, "model": tok.rq_vae.state_dict()}, root + "rqvae.pt")
    cfg["pretrained_rqvae_path"] = root + "rqvae.pt"
    torch.manual_seed(0)
    out = train_decoder.train(**cfg)
    return cfg, out["checkpoint"], root


def test_exact_metrics_do_not_depend_on_the_seed(trained):
    import evaluate_decoder
    cfg, checkpoint, _ = trained
    results = []
    for seed in (1, 2):
        torch.manual_seed(seed)
        results.append(evaluate_decoder.evaluate(**_eval_config(cfg, checkpoint_path=checkpoint, beam_impl="exact")))
    assert results[0] == results[1]
    res = results[0]
    assert set(res) == KEYS and res["users"] == USERS
    assert all(0.0 <= v <= 1.0 for name, v in res.items() if name != "users")
    assert res["h@1"] <= res["h@5"] <= res["h@10"]
    # max_batches stops early: two batches of 16 users
    part = evaluate_decoder.evaluate(**_eval_config(cfg, checkpoint_path=checkpoint, max_batches=2))
    assert part["users"] == 32


def test_the_sampling_search_and_the_operator_paths_run_too(trained):
    import evaluate_decoder
    cfg, checkpoint, _ = trained
    torch.manual_seed(3)
    res = evaluate_decoder.evaluate(**_eval_config(cfg, checkpoint_path=checkpoint, beam_impl="sample", attention_impl="torch",
                                                   norm_impl="torch", ffn_impl="torch", embed_impl="torch"))
    assert set(res) == KEYS and res["users"] == USERS
    assert all(0.0 <= v <= 1.0 for name, v in res.items() if name != "users")


def test_a_checkpoint_of_another_corpus_is_rejected(trained):
    import evaluate_decoder
    cfg, checkpoint, root = trained
    state = torch.load(checkpoint, map_location="cpu", weights_only=False)
    state["model"]["codebooks"] = (state["model"]["codebooks"] + 1) % cfg["vae_codebook_size"]
    torch.save(state, root + "other_corpus.pt")
    with pytest.raises(ValueError, match="corpus ids differ"):
        evaluate_decoder.evaluate(**_eval_config(cfg, checkpoint_path=root + "other_corpus.pt"))
    with pytest.raises(ValueError, match="checkpoint_path"):
        evaluate_decoder.evaluate(**_eval_config(cfg))
