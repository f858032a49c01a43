"""The exact constrained beam search on the host: the argument checks of rqhip_beam_topk_step (all of them run before
any HIP call), ops.beam_topk_step's signature, model.beam_impl and the errors of `generate`, and the evaluation entry
point (evaluate_decoder.evaluate, configs/decoder_amazon_eval.gin).  No GPU needed."""
import ctypes
import inspect
import os

import pytest
import torch

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rq-vae-recommender_amd")


def _topk(l, *, h=0, B=4, beams_in=1, K=256, k=10, H=3, N=0, ld_logits=None, parents=False, index=None, index_bytes=0):
    return l.rqhip_beam_topk_step(None, K if ld_logits is None else ld_logits, 1 if parents else None,
                                  1 if parents else None, h, B, beams_in, K, k, index, index_bytes, None, N, H, H, None,
                                  None, None, None)


def test_beam_topk_step_argument_checks_without_gpu():
    from rqhip import _lib
    l = _lib.lib()
    err = l.rqhip_last_error
    assert _topk(l, K=4097) == -2 and b"K <= 4096" in err()
    assert _topk(l, k=65) == -2 and b"k <= 64" in err()
    assert _topk(l, h=1, beams_in=65, parents=True) == -2 and b"beams_in <= 64" in err()
    assert _topk(l, K=8, k=9) == -1 and b"candidates" in err()                            # k > beams_in * K at h = 0
    assert _topk(l, h=1, beams_in=2, K=8, k=17, parents=True) == -1 and b"candidates" in err()
    assert _topk(l, h=0, beams_in=2) == -1 and b"beams_in = 1" in err()                   # one row per user at h = 0
    assert _topk(l, h=3, beams_in=10, H=3, parents=True) == -1 and b"id levels" in err()  # h + 1 > H
    assert _topk(l, h=16, beams_in=10, H=16, parents=True) == -2 and b"RQHIP_MAX_PREFIX_LEN" in err()
    assert _topk(l, ld_logits=100) == -1 and b"ld_logits" in err()
    assert _topk(l, N=5) == -1 and b"bad corpus" in err()                                 # null corpus
    assert _topk(l) == -1 and b"null pointer" in err()                                    # null logits
    assert _topk(l, h=1, beams_in=10) == -1 and b"null pointer" in err()                  # null parents at h > 0
    # the index: none, one byte short, and large enough (B = 0 then returns OK before any launch)
    need = l.rqhip_prefix_index_bytes(0, 3)
    assert need > 0
    buf = ctypes.create_string_buffer(need)
    assert _topk(l, B=0) == -3 and b"index buffer too small" in err()
    assert _topk(l, B=0, index=ctypes.addressof(buf), index_bytes=need - 1) == -3 and b"index buffer too small" in err()
    assert _topk(l, B=0, index=ctypes.addressof(buf), index_bytes=need) == 0
    assert _topk(l, B=0, K=8, k=64, h=1, beams_in=64, parents=True, index=ctypes.addressof(buf), index_bytes=need) == 0
    assert l.rqhip_version() == 462


def test_ops_beam_topk_step_signature():
    from rqhip import ops
    assert list(inspect.signature(ops.beam_topk_step).parameters) == ["logits", "parent_scores", "parent_ids", "index",
                                                                      "corpus", "k"]


def _model(K=8, k=4):
    from modules.model import EncoderDecoderRetrievalModel
    return EncoderDecoderRetrievalModel(torch.zeros(4, 3, dtype=torch.long), 3, K, t5_d_model=8, t5_num_heads=1, t5_d_ff=8,
                                        t5_num_layers=1, top_k_for_generation=k)


def test_beam_impl_defaults_to_sample():
    assert _model().beam_impl == "sample"


def test_generate_rejects_bad_beam_settings_before_any_device_work():
    from rqhip._lib import RqHipError
    args = (torch.ones(1, 3, dtype=torch.long), torch.zeros(1, 3, dtype=torch.long))
    m = _model()
    m.beam_impl = "nope"
    with pytest.raises(ValueError, match="beam_impl"):
        m.generate(*args)
    m = _model(K=8, k=9)
    m.beam_impl = "exact"
    with pytest.raises(ValueError, match="K=8"):
        m.generate(*args)
    # k <= K is enough under "exact" (K = 128 > n_cands = 64), and CPU tensors still get the no-CPU-path error
    m = _model(K=128, k=100)
    with pytest.raises(ValueError, match="n_cands"):
        m.generate(*args)
    m.beam_impl = "exact"
    with pytest.raises(RqHipError, match="ROCm device tensors"):
        m.generate(*args)


SHARED_WITH_TRAIN = ["batch_size", "dataset_folder", "dataset", "pretrained_rqvae_path", "force_dataset_process", "vae_input_dim",
                     "vae_embed_dim", "vae_hidden_dims", "vae_codebook_size", "vae_codebook_normalize", "vae_sim_vq",
                     "vae_n_cat_feats", "vae_n_layers", "dataset_split", "t5_d_model", "t5_num_heads", "t5_d_ff",
                     "t5_num_layers", "top_k_for_generation", "should_add_sep_token", "num_user_bins", "top_k_eval_list",
                     "norm_impl", "ffn_impl", "embed_impl"]
OWN = dict(checkpoint_path=None, beam_impl="exact", attention_impl="hip", max_batches=None)


def test_evaluate_signature_has_trains_parameters_and_defaults():
    import evaluate_decoder
    import train_decoder
    params = inspect.signature(evaluate_decoder.evaluate).parameters
    train = inspect.signature(train_decoder.train).parameters
    assert set(params) == set(SHARED_WITH_TRAIN) | set(OWN)
    for name in SHARED_WITH_TRAIN:
        assert params[name].default == train[name].default, name
    for name, default in OWN.items():
        assert params[name].default == default, name


def test_eval_config_parses_and_binds_only_evaluate_parameters():
    import evaluate_decoder
    from data.processed import RecDataset
    from rqhip import ginlite
    params = inspect.signature(evaluate_decoder.evaluate).parameters

    def bindings(name):
        ginlite.clear_config()
        try:
            ginlite.parse_config_file(os.path.join(PKG, "configs", name))
            return {scope: dict(b) for scope, b in ginlite._BINDINGS.items()}
        finally:
            ginlite.clear_config()

    got = bindings("decoder_amazon_eval.gin")
    assert set(got) == {"evaluate"}
    bound = got["evaluate"]
    assert set(bound) <= set(params)
    assert bound["dataset"] is RecDataset.AMAZON and bound["beam_impl"] == "exact" and bound["attention_impl"] == "hip"
    # the Amazon values of decoder_amazon.gin, wherever both bind a parameter (the kernels of training apart)
    train = bindings("decoder_amazon.gin")["train"]
    shared = (set(bound) & set(train)) - {"attention_impl"}
    assert {"vae_hidden_dims", "vae_codebook_size", "t5_d_model", "t5_num_layers", "batch_size", "dataset_folder",
            "pretrained_rqvae_path", "top_k_for_generation"} <= shared
    assert {n: bound[n] for n in shared} == {n: train[n] for n in shared}
