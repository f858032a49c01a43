"""The host side of the retrieval model's input path (no GPU): the window law against the reference's slicing, SeqData's
sources and checks, the argument checks of rqhip_seq_batch, train_decoder.train's signature and configuration, and the
checkpoint loader."""
import inspect
import os

import pytest
import torch

from conftest import PKG

BIG = 2 ** 62


def _reference_rows(seq, S):
    """{(start, end): (history, target)} over the reference's two inclusive ranges, sliced as it writes them:
    start = randint(0, max(0, len(seq) - 3)), end = randint(start + 3, start + S + 1), sample = seq[start:end]."""
    out = {}
    for start in range(0, max(0, len(seq) - 3) + 1):
        for end in range(start + 3, start + S + 1 + 1):
            sample = seq[start:end]
            out[(start, end)] = (sample[:-1], sample[-1])
    return out


@pytest.mark.parametrize("S", [2, 3, 20])
def test_seq_window_is_the_reference_slicing(S):
    from data.processed import seq_window
    for n_hist in range(0, S + 4):
        seq = list(range(100, 100 + n_hist)) + [999]
        n = len(seq)
        want = _reference_rows(seq, S)
        seen = []
        m0, m1 = max(0, n - 3) + 1, S - 1
        for u0 in range(m0):
            for u1 in range(m1):
                first, count, fut_pos = seq_window(n_hist, u0, u1, S, True)
                pair = (u0, u0 + 3 + u1)                       # the (start, end) these two draws stand for
                seen.append(pair)
                hist, target = want[pair]
                assert seq[first:first + count] == hist and seq[fut_pos] == target, (S, n_hist, u0, u1)
                assert 0 <= count <= S and first + count == fut_pos
                # only the residue matters: the largest draws below 2^62 with the same residues
                b0, b1 = u0 + m0 * ((BIG - 1 - u0) // m0), u1 + m1 * ((BIG - 1 - u1) // m1)
                assert BIG - m0 <= b0 < BIG and BIG - m1 <= b1 < BIG
                assert seq_window(n_hist, b0, b1, S, True) == (first, count, fut_pos)
        # every pair of the reference's ranges exactly once: uniform draws give the reference's distribution
        assert len(seen) == len(set(seen)) and sorted(seen) == sorted(want)
        first, count, fut_pos = seq_window(n_hist, 5, 7, S, False)
        assert seq[first:first + count] == seq[:-1][-S:] and seq[fut_pos] == 999
        assert count == min(S, n_hist)


def test_seq_window_rejects_bad_sizes():
    from data.processed import seq_window
    with pytest.raises(ValueError):
        seq_window(3, 0, 0, 1, True)
    with pytest.raises(ValueError):
        seq_window(-1, 0, 0, 20, False)


def _split(hists, futs, users=None):
    offsets = torch.zeros(len(hists) + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(torch.tensor([len(h) for h in hists]), 0)
    return {"userId": torch.tensor(users if users is not None else list(range(len(hists))), dtype=torch.int64),
            "offsets": offsets, "items": torch.tensor([i for h in hists for i in h], dtype=torch.int64),
            "itemId_fut": torch.tensor(futs, dtype=torch.int64)}


HISTS = [[3, 1, 4], [], [5] * 2 + list(range(10, 32)), [7]]
FUTS = [9, 2, 6, 8]


def _sequences():
    return {"train": _split(HISTS, FUTS, users=[40, 41, 42, 43]), "eval": _split([[1]], [2]), "test": _split([[2, 3]], [4])}


def test_seq_data_loads_a_sequences_file(tmp_path):
    from data.processed import RecDataset, SeqData
    torch.save(_sequences(), tmp_path / "sequences.pt")
    ds = SeqData(str(tmp_path), dataset=RecDataset.AMAZON, is_train=True, split="beauty")
    assert len(ds) == 4 and ds.max_seq_len == 20 and not ds.synthetic and not ds.subsample
    assert ds.offsets.tolist() == [0, 3, 3, 27, 28] and ds.items.dtype == torch.int64
    test = SeqData(str(tmp_path), dataset=RecDataset.AMAZON, is_train=False)
    assert len(test) == 1 and test.items.tolist() == [2, 3] and test.split == "test"
    assert SeqData(str(tmp_path), dataset=RecDataset.ML_1M).max_seq_len == 200
    assert SeqData(str(tmp_path), dataset=RecDataset.ML_32M).max_seq_len == 200
    with pytest.raises(AssertionError, match="subsample"):
        SeqData(str(tmp_path), dataset=RecDataset.AMAZON, is_train=False, subsample=True)


def test_seq_data_getitem_without_subsample_is_the_hand_written_row():
    from data.processed import RecDataset, SeqData
    ds = SeqData("/nonexistent", dataset=RecDataset.AMAZON, sequences=_sequences())
    pad = [-1] * 20
    rows = {0: ([3, 1, 4] + pad[:17], 9, 40), 1: (pad, 2, 41), 2: (([5] * 2 + list(range(10, 32)))[-20:], 6, 42),
            3: ([7] + pad[:19], 8, 43)}
    for i, (ids, fut, user) in rows.items():
        b = ds[i]
        assert b.ids.tolist() == ids and b.ids_fut.tolist() == [fut] and b.user_ids.tolist() == [user]
        assert b.seq_mask.tolist() == [v >= 0 for v in ids] and b.seq_mask.dtype == torch.bool
        assert b.x.tolist() == [-1] * 20 and b.x_fut.tolist() == [-1]          # placeholders without an item matrix
    # with an item matrix the features are gathered, -1 at padded positions
    matrix = torch.arange(40 * 768, dtype=torch.float32).reshape(40, 768)
    b = SeqData("/nonexistent", dataset=RecDataset.AMAZON, sequences=_sequences(), item_matrix=matrix)[0]
    assert b.x.shape == (20, 768) and torch.equal(b.x[:3], matrix[[3, 1, 4]]) and bool((b.x[3:] == -1).all())
    assert torch.equal(b.x_fut, matrix[[9]])


def test_seq_data_getitem_with_subsample_follows_seq_window():
    from data.processed import RecDataset, SeqData, seq_window
    ds = SeqData("/nonexistent", dataset=RecDataset.AMAZON, sequences=_sequences(), subsample=True)
    seq = HISTS[2] + [FUTS[2]]
    torch.manual_seed(3)
    u0, u1 = torch.randint(0, 2 ** 62, (2,)).tolist()
    first, count, fut_pos = seq_window(len(HISTS[2]), u0, u1, 20, True)
    torch.manual_seed(3)
    b = ds[2]
    assert b.ids.tolist() == seq[first:first + count] + [-1] * (20 - count) and b.ids_fut.tolist() == [seq[fut_pos]]


def test_seq_data_synthetic_opt_in_and_missing_file(tmp_path, capsys):
    from data.processed import RecDataset, SeqData
    ds = SeqData("synthetic:300", dataset=RecDataset.AMAZON, subsample=True)
    assert ds.synthetic and "SYNTHETIC" in capsys.readouterr().out
    assert len(ds) == 150 and SeqData("synthetic:20", dataset=RecDataset.AMAZON).__len__() == 64
    lengths = ds.offsets[1:] - ds.offsets[:-1]
    assert int(lengths.min()) >= 1 and int(lengths.min()) < 19 and 21 < int(lengths.max()) <= 40   # short and long rows
    again = SeqData("synthetic:300", dataset=RecDataset.AMAZON)
    assert torch.equal(again.items, ds.items) and torch.equal(again.itemId_fut, ds.itemId_fut)      # deterministic
    ds.check_items(300)
    with pytest.raises(FileNotFoundError, match=r"sequences\.pt not found.*INTEGRATION\.md.*synthetic:<n>"):
        SeqData(str(tmp_path), dataset=RecDataset.AMAZON)


def test_check_items():
    from data.processed import RecDataset, SeqData
    ds = SeqData("/nonexistent", dataset=RecDataset.AMAZON, sequences=_sequences())
    ds.check_items(32)
    with pytest.raises(ValueError, match="outside"):
        ds.check_items(31)                       # the largest stored id is 31: an id equal to n_items
    bad = _sequences()
    bad["train"]["items"][1] = -1
    with pytest.raises(ValueError, match="outside"):
        SeqData("/nonexistent", dataset=RecDataset.AMAZON, sequences=bad).check_items(32)
    bad = _sequences()
    bad["train"]["itemId_fut"][0] = 32
    with pytest.raises(ValueError, match="itemId_fut"):
        SeqData("/nonexistent", dataset=RecDataset.AMAZON, sequences=bad).check_items(32)


def test_seq_batch_argument_checks_without_gpu():
    from rqhip import _lib
    l = _lib.lib()
    assert l.rqhip_seq_batch_supported(2, 2) == 1 and l.rqhip_seq_batch_supported(9, 256) == 1
    assert l.rqhip_seq_batch_supported(5, 20) == 1
    for w, S in ((1, 20), (10, 20), (4, 1), (4, 257)):
        assert l.rqhip_seq_batch_supported(w, S) == 0

    def call(B=4, w=4, S=20, U=3, nnz=5, n_items=7, null=()):
        # non-null placeholders are never dereferenced: every case below is rejected before any HIP call
        p = {name: (None if name in null else 64) for name in
             ("offsets", "items", "fut", "user", "rows", "draws", "table", "sem_ids", "seq_mask", "sem_ids_fut", "user_ids",
              "token_type", "token_type_fut")}
        return l.rqhip_seq_batch(p["offsets"], p["items"], p["fut"], p["user"], U, nnz, p["rows"], B, p["draws"], p["table"],
                                 n_items, w, S, p["sem_ids"], p["seq_mask"], p["sem_ids_fut"], p["user_ids"], p["token_type"],
                                 p["token_type_fut"], None)

    for name in ("offsets", "items", "fut", "user", "rows", "table", "sem_ids", "seq_mask", "sem_ids_fut", "user_ids"):
        assert call(null=(name,)) == -1, name
        assert b"null pointer" in l.rqhip_last_error(), name
    for w, S in ((1, 20), (10, 20), (4, 1), (4, 257)):
        assert call(w=w, S=S) == -1
        assert b"only w in 2 .. 9 and S in 2 .. 256" in l.rqhip_last_error()
    assert call(B=-1) == -1 and b"bad sizes" in l.rqhip_last_error()
    assert call(U=-1) == -1 and call(nnz=-1) == -1 and call(n_items=-1) == -1
    everything = ("offsets", "items", "fut", "user", "rows", "draws", "table", "sem_ids", "seq_mask", "sem_ids_fut",
                  "user_ids", "token_type", "token_type_fut")
    assert call(B=0, null=everything) == 0                       # empty batch: nothing to do
    assert call(B=0, w=1, null=everything) == -1                 # the shape is still checked


def test_ops_seq_batch_rejects_host_tensors_and_bad_shapes():
    from data.processed import RecDataset, SeqData
    from rqhip import ops
    ds = SeqData("/nonexistent", dataset=RecDataset.AMAZON, sequences=_sequences())
    table = torch.zeros(32, 4, dtype=torch.int64)
    rows = torch.tensor([0, 1])
    assert ops.seq_batch_supported(4, 20) and not ops.seq_batch_supported(4, 300)
    with pytest.raises(ops.RqHipError, match="ROCm device tensors"):
        ops.seq_batch(ds, rows, table, 20)
    with pytest.raises(ops.RqHipError, match="draws"):
        ops.seq_batch(ds, rows, table, 20, draws=torch.zeros(3, 2, dtype=torch.int64))
    with pytest.raises(ops.RqHipError, match="table"):
        ops.seq_batch(ds, rows, table.float(), 20)
    with pytest.raises(ops.RqHipError, match="not supported"):
        ops.seq_batch(ds, rows, torch.zeros(32, 10, dtype=torch.int64), 20)


# every parameter of the reference's train_decoder.train with its default
REFERENCE_TRAIN = dict(
    iterations=500000, batch_size=64, learning_rate=0.001, weight_decay=0.01, dataset_folder="dataset/ml-1m",
    save_dir_root="out/", dataset="ML_1M", pretrained_rqvae_path=None, pretrained_decoder_path=None, split_batches=True,
    amp=False, wandb_logging=False, force_dataset_process=False, mixed_precision_type="fp16", gradient_accumulate_every=1,
    save_model_every=1000000, partial_eval_every=1000, full_eval_every=10000, vae_input_dim=18, vae_embed_dim=16,
    vae_hidden_dims=[18, 18], vae_codebook_size=32, vae_codebook_normalize=False, vae_sim_vq=False, vae_n_cat_feats=18,
    vae_n_layers=3, dataset_split="beauty", push_vae_to_hf=False, train_data_subsample=True,
    vae_hf_model_name="edobotta/rqvae-amazon-beauty", max_grad_norm=None, t5_d_model=128, t5_num_heads=6, t5_d_ff=1024,
    t5_num_layers=4, top_k_for_generation=10, should_add_sep_token=True, num_user_bins=None, top_k_eval_list=[1, 5, 10])
ADDED_TRAIN = dict(attention_impl="hip_train", norm_impl="hip", ffn_impl="hip", head_impl="hip", embed_impl="hip",
                   log_every=100)


def test_train_signature_has_the_reference_parameters():
    import train_decoder
    from data.processed import RecDataset
    params = inspect.signature(train_decoder.train).parameters
    want = dict(REFERENCE_TRAIN, dataset=RecDataset.ML_1M)
    for name, default in {**want, **ADDED_TRAIN}.items():
        assert name in params, name
        assert params[name].default == default, name
    assert list(params)[:len(want)] == list(want)                # in the reference's order, the additions behind them
    assert set(params) == set(want) | set(ADDED_TRAIN)


def test_decoder_config_parses_and_binds_only_train_parameters():
    import train_decoder
    from data.processed import RecDataset
    from rqhip import ginlite
    params = inspect.signature(train_decoder.train).parameters
    ginlite.clear_config()
    try:
        ginlite.parse_config_file(os.path.join(PKG, "configs", "decoder_amazon.gin"))
        assert set(ginlite._BINDINGS) == {"train"}
        bound = dict(ginlite._BINDINGS["train"])
    finally:
        ginlite.clear_config()
    assert set(bound) <= set(params)
    assert bound["dataset"] is RecDataset.AMAZON and bound["batch_size"] == 640 and bound["t5_d_model"] == 384
    assert bound["vae_hidden_dims"] == [512, 256, 128] and bound["vae_n_layers"] == 3 and bound["vae_codebook_size"] == 256
    assert {k: bound[k] for k in ADDED_TRAIN if k != "log_every"} == {k: v for k, v in ADDED_TRAIN.items() if k != "log_every"}


def test_rejected_settings_raise_before_any_gpu_work():
    import train_decoder
    from data.processed import RecDataset
    with pytest.raises(Exception, match="not supported"):
        train_decoder.train(dataset=RecDataset.ML_1M)
    with pytest.raises(NotImplementedError, match="fp32"):
        train_decoder.train(dataset=RecDataset.AMAZON, amp=True)
    with pytest.raises(NotImplementedError, match="network"):
        train_decoder.train(dataset=RecDataset.AMAZON, push_vae_to_hf=True)


def test_checkpoint_loading_strips_the_compile_prefix(tmp_path):
    import train_decoder
    from retrieval_cases import tiny_model
    src, dst = tiny_model(), tiny_model()
    with torch.no_grad():
        for p in src.parameters():
            p.add_(1.0)
    sd = src.state_dict()
    assert train_decoder.strip_compile_prefix({"_orig_mod.a._orig_mod.b": 1, "c": 2}) == {"a._orig_mod.b": 1, "c": 2}
    for name, prefixed in (("compiled.pt", {"_orig_mod." + k: v for k, v in sd.items()}), ("plain.pt", sd)):
        torch.save({"iter": 41, "model": prefixed}, tmp_path / name)
        dst.load_state_dict(tiny_model().state_dict())
        assert train_decoder.load_checkpoint(str(tmp_path / name), dst) == 42
        for k, v in dst.state_dict().items():
            assert torch.equal(v, sd[k]), k
