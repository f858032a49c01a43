"""train_decoder.train end to end on a synthetic corpus at the smallest shapes the kernels implement: a short run, its
checkpoint, a resumed run, the fused paths it takes, and the settings it rejects."""
import pytest
import torch

pytestmark = pytest.mark.gpu

KS = [1, 5, 10]
USERS = 150                     # data.processed.synthetic_sequences: max(64, 300 // 2) per split
BATCHES = -(-USERS // 16)       # of one pass over the eval split


def _config(**over):
    from data.processed import RecDataset
    cfg = dict(dataset_folder="synthetic:300", dataset=RecDataset.AMAZON, batch_size=16, iterations=8, partial_eval_every=4,
               full_eval_every=8, log_every=1, learning_rate=0.001, weight_decay=0.0001, max_grad_norm=1.0,
               vae_input_dim=768, vae_hidden_dims=[32], vae_embed_dim=16, vae_codebook_size=16, vae_n_layers=3,
               vae_n_cat_feats=0, t5_d_model=64, t5_num_heads=2, t5_d_ff=128, t5_num_layers=2, top_k_for_generation=10,
               top_k_eval_list=KS)
    cfg.update(over)
    return cfg


def _counted_run(**cfg):
    """train(**cfg) with the calls of ops.seq_batch, ops.sid_embed_fwd and ops.sid_embed_bwd counted."""
    import train_decoder
    from rqhip import ops
    calls = {"seq_batch": 0, "sid_embed_fwd": 0, "sid_embed_bwd": 0}
    with pytest.MonkeyPatch.context() as mp:
        for name in calls:
            def counted(*a, _name=name, _real=getattr(ops, name), **kw):
                calls[_name] += 1
                return _real(*a, **kw)
            mp.setattr(ops, name, counted)
        torch.manual_seed(0)
        return train_decoder.train(**cfg), calls


@pytest.fixture(scope="module")
def short_run(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("decoder")) + "/"
    out, calls = _counted_run(**_config(save_dir_root=root))
    return out, calls, root


def test_a_short_run_logs_evaluates_and_saves(short_run):
    import os
    from modules.model import EncoderDecoderRetrievalModel
    out, _, root = short_run
    assert (out["start_iter"], out["end_iter"]) == (0, 8)
    assert [it for it, _ in out["losses"]] == list(range(8))
    assert all(torch.isfinite(torch.tensor(v)) for _, v in out["losses"])
    assert [it for it, _ in out["eval_losses"]] == [3, 7] and all(v == v and abs(v) != float("inf") for _, v in out["eval_losses"])
    assert set(out["eval_metrics"]) == {"ndcg"} | {f"h@{k}" for k in KS}
    assert all(0.0 <= v <= 1.0 for v in out["eval_metrics"].values())
    assert out["checkpoint"] == root + "checkpoint_7.pt" and os.path.exists(out["checkpoint"])
    state = torch.load(out["checkpoint"], map_location="cpu", weights_only=False)
    assert {"iter", "model", "optimizer", "scheduler"} <= set(state) and state["iter"] == 7
    fresh = EncoderDecoderRetrievalModel(torch.zeros_like(state["model"]["codebooks"]), 3, 16, t5_d_model=64, t5_num_heads=2,
                                         t5_d_ff=128, t5_num_layers=2)
    fresh.load_state_dict(state["model"], strict=True)
    # step 8 lies inside the warm-up of the inverse-square-root schedule: the device's rate is the base rate in fp32
    assert state["scheduler"]["last_epoch"] == 8 and state["scheduler"]["warmup_steps"] == 10000
    assert out["learning_rate"] == torch.tensor(0.001, dtype=torch.float32).item()
    steps = {float(s["step"]) for s in state["optimizer"]["state"].values()}
    assert steps == {8.0}


def test_the_fused_paths_are_taken(short_run):
    _, calls, _ = short_run
    # one launch per batch: 8 training batches, two partial evals and one full eval over the eval split
    assert calls["seq_batch"] == 8 + 3 * BATCHES
    # the encoder's and the decoder's front per forward (training and partial eval), the encoder's per generate
    assert calls["sid_embed_fwd"] == 2 * 8 + 2 * 2 * BATCHES + BATCHES
    assert calls["sid_embed_bwd"] == 2 * 8


def test_resume_continues_from_the_checkpoint(short_run, tmp_path):
    import train_decoder
    first, _, _ = short_run
    root = str(tmp_path) + "/"
    torch.manual_seed(0)         # the first run's seed: the same random RQ-VAE, so the same id table
    out = train_decoder.train(**_config(save_dir_root=root, pretrained_decoder_path=first["checkpoint"], iterations=2,
                                        partial_eval_every=100, full_eval_every=100))
    assert (out["start_iter"], out["end_iter"]) == (8, 10) and [it for it, _ in out["losses"]] == [8, 9]
    assert out["checkpoint"] == root + "checkpoint_9.pt"
    state = torch.load(out["checkpoint"], map_location="cpu", weights_only=False)
    # the counters went on from the saved ones: optimizer and scheduler state were loaded
    assert state["iter"] == 9 and state["scheduler"]["last_epoch"] == 10
    assert {float(s["step"]) for s in state["optimizer"]["state"].values()} == {10.0}
    assert out["eval_losses"] == [] and out["eval_metrics"] == {}
    # and the weights: the resumed run starts below the loss the untrained model had on the same id table
    assert out["losses"][0][1] < first["losses"][0][1]


def test_the_operator_paths_run_too(tmp_path):
    out, calls = _counted_run(**_config(save_dir_root=str(tmp_path) + "/", iterations=2, partial_eval_every=2, full_eval_every=2,
                                        attention_impl="torch", norm_impl="torch", ffn_impl="torch", head_impl="torch",
                                        embed_impl="torch"))
    assert calls["sid_embed_fwd"] == 0 and calls["sid_embed_bwd"] == 0
    assert calls["seq_batch"] == 2 + 2 * BATCHES                 # the batches are built the same way
    assert len(out["losses"]) == 2 and all(v == v for _, v in out["losses"])
    assert set(out["eval_metrics"]) == {"ndcg"} | {f"h@{k}" for k in KS}


def test_rejected_settings():
    import train_decoder
    from data.processed import RecDataset
    with pytest.raises(NotImplementedError, match="fp32"):
        train_decoder.train(**_config(amp=True))
    with pytest.raises(Exception, match="not supported"):
        train_decoder.train(**_config(dataset=RecDataset.ML_1M))
    with pytest.raises(NotImplementedError, match="network"):
        train_decoder.train(**_config(push_vae_to_hf=True))
