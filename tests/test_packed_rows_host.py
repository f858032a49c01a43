"""The host side of packed encoder rows (modules/model.py: encoder_rows = "packed"): the vectorised window law, the
batch type that carries the rows' item counts, the model attribute and what it leaves alone.  No GPU needed."""
import pytest
import torch

from retrieval_cases import tiny_batch, tiny_model


def _draws(n, seed):
    g = torch.Generator().manual_seed(seed)
    u = torch.randint(0, 2 ** 62, (n, 2), generator=g, dtype=torch.int64)
    u[0] = 0
    u[1] = 2 ** 62 - 1
    u[2, 0], u[2, 1] = 0, 2 ** 62 - 1
    u[3, 0], u[3, 1] = 2 ** 62 - 1, 0
    return u


@pytest.mark.parametrize("S", [2, 20])
@pytest.mark.parametrize("subsample", [False, True])
def test_seq_window_counts_is_seq_window(S, subsample):
    from data.processed import seq_window, seq_window_counts
    draws = _draws(300, 7 + S)
    for n_hist in range(46):
        want = torch.tensor([seq_window(n_hist, int(u0), int(u1), S, subsample)[1] for u0, u1 in draws.tolist()])
        got = seq_window_counts(torch.full((draws.shape[0],), n_hist, dtype=torch.int64), draws if subsample else None, S,
                                subsample)
        assert got.dtype == torch.int64 and torch.equal(got, want), (n_hist, S, subsample)
    # mixed lengths in one call, as a batch has them
    n_hist = torch.arange(300) % 46
    want = torch.tensor([seq_window(int(n), int(u0), int(u1), S, subsample)[1]
                         for n, (u0, u1) in zip(n_hist.tolist(), draws.tolist())])
    assert torch.equal(seq_window_counts(n_hist, draws if subsample else None, S, subsample), want)


def test_seq_window_counts_rejects_what_seq_window_rejects():
    from data.processed import seq_window_counts
    with pytest.raises(ValueError):
        seq_window_counts(torch.tensor([3]), None, 1, False)
    with pytest.raises(ValueError):
        seq_window_counts(torch.tensor([-1]), None, 20, False)


def test_counted_batch_is_a_tokenized_batch():
    from data.schemas import CountedSeqBatch, TokenizedSeqBatch
    plain = tiny_batch()
    counts = torch.tensor([2, 1])
    batch = CountedSeqBatch(*plain, item_counts=counts)
    assert isinstance(batch, TokenizedSeqBatch) and isinstance(batch, tuple)
    assert CountedSeqBatch._fields == TokenizedSeqBatch._fields and len(batch) == 6
    user_ids, sem_ids, sem_ids_fut, seq_mask, tt, tt_fut = batch            # positional unpacking
    assert sem_ids is plain.sem_ids and seq_mask is plain.seq_mask and tt is None and tt_fut is None
    assert batch.sem_ids_fut is plain.sem_ids_fut and batch.user_ids is user_ids
    assert batch.item_counts is counts
    assert tuple(batch) == tuple(plain)
    replaced = batch._replace(token_type_ids=sem_ids)
    assert isinstance(replaced, CountedSeqBatch) and replaced.item_counts is counts and replaced.token_type_ids is sem_ids
    assert CountedSeqBatch(*plain).item_counts is None
    assert not hasattr(plain, "item_counts")


def test_encoder_rows_attribute():
    from modules.model import ENCODER_ROWS
    model = tiny_model()
    assert ENCODER_ROWS == ("padded", "packed") and model.encoder_rows == "padded"
    keys = set(model.state_dict())
    model.encoder_rows = "packed"
    assert set(model.state_dict()) == keys and not any("encoder_rows" in k for k in keys)
    # on the host (no device batch) "packed" runs the padded path, silently, like every other *_impl
    from data.schemas import CountedSeqBatch
    plain = tiny_batch()
    counted = CountedSeqBatch(*plain, item_counts=torch.tensor([2, 2]))
    model.eval()
    with torch.no_grad():
        assert torch.equal(model(counted).loss, model(plain).loss)
    model.encoder_rows = "ragged"
    for batch in (plain, counted):
        with pytest.raises(ValueError, match="encoder_rows"):
            model(batch)


def test_stack_attributes_unchanged():
    from modules import t5
    assert list(t5.STACK_ATTRIBUTES) == ["attention_impl", "attention_long_impl", "norm_impl", "ffn_impl", "proj_impl",
                                         "matmul_arith", "attention_arith", "weight_images", "saved_activations"]
    assert "encoder_rows" not in t5.STACK_ATTRIBUTES
    assert t5.PackedRows._fields == ("cu", "bound", "batch", "rows")


def test_train_decoder_reads_encoder_rows_from_its_own_configurable():
    """`train`'s parameter set is pinned (tests/test_seq_batch_host.py), so the choice is the configurable
    train_decoder.encoder_rows(mode), bound as `encoder_rows.mode`."""
    import inspect

    import train_decoder
    gin = train_decoder.gin
    assert "encoder_rows" not in inspect.signature(train_decoder.train).parameters
    assert train_decoder.encoder_rows() == "padded" and train_decoder.encoder_rows(mode="packed") == "packed"
    gin.clear_config()
    try:
        gin.parse_config('encoder_rows.mode = "packed"')
        assert train_decoder.encoder_rows() == "packed"
        gin.parse_config('encoder_rows.mode = "ragged"')
        with pytest.raises(ValueError, match="encoder_rows"):
            train_decoder.encoder_rows()
        with pytest.raises(ValueError, match="encoder_rows"):      # before any data or GPU work
            train_decoder.train(dataset=train_decoder.RecDataset.AMAZON)
    finally:
        gin.clear_config()
    assert train_decoder.encoder_rows() == "padded"


def test_packed_config_is_the_base_config_plus_one_line():
    import os

    from conftest import ROOT
    cfg = os.path.join(ROOT, "rq-vae-recommender_amd", "configs")

    def bindings(name):
        return [l.strip() for l in open(os.path.join(cfg, name)) if l.strip() and not l.startswith("#")]

    base, packed = bindings("decoder_amazon.gin"), bindings("decoder_amazon_packed.gin")
    assert [l for l in packed if l not in base] == ['encoder_rows.mode="packed"']
    assert [l for l in base if l not in packed] == []
