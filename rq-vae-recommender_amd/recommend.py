"""`python recommend.py <config.gin>` -- the items one train_decoder.py checkpoint recommends on the eval split, and
the retrieval metrics at the level of ITEMS next to those at the level of semantic-id tuples.

The retrieval model generates tuples of semantic ids; several corpus items can share a tuple, and the tokenizer tells
them apart by a dedup column the decoder never generates.  evaluate_decoder.evaluate therefore counts a hit when a
generated tuple equals the target's tuple -- as if one of the items that share it had been named.  Here every batch goes
through `model.recommend_items`: one `generate_next_sem_id` call and ONE launch (csrc/sid_items.hip) that expands each
user's beams, best first, to the corpus items that carry them, in ascending item number, cut at `n_items`.

The gin-configurable `recommend(...)` takes every parameter of evaluate_decoder.evaluate under the same name and default,
builds the item set, the eval split and the tokenizer and loads the checkpoint exactly as `evaluate` does (the same
corpus check), and runs the eval split ONCE in a fixed order.  Its own parameters:

  n_items          items returned per user (default 10, at most 256).
  exclude_history  (default True) the items of a user's own history, batch.sem_ids with its dedup column, are never
                   recommended.  A user whose target item is among their own history items can then not be hit at the
                   item level: `targets_in_history` counts those users, so that the item metrics can be read against it.
  output_path      when given, torch.save of {"items": int64 [U, n_items] (-1 padded), "scores": fp32 [U, n_items]
                   (-inf padded)} in the order of the eval split.

It returns {"item": {...}, "sid": {...}, "users": U, "targets_in_history": count}: "item" holds `ndcg` and `h@k` of the
target ITEM among the recommended items, "sid" those of the target TUPLE among the generated tuples -- what `evaluate`
reports, from the same `generate` call.  Without exclude_history an item hit at position p implies a tuple hit at a
position <= p, so every item h@k is at most the tuple h@k; the gap is what tuple collisions hide.  The target item is
the corpus row with the target's tuple and dedup rank; a target that is no corpus row cannot be scored, so the run
raises when it meets one (counted on the device, read once at the end with the metrics).  One process, one GPU.

Packed encoder rows: as evaluate_decoder.evaluate, `recommend` reads the binding `encoder_rows.mode` of
train_decoder.encoder_rows before any other work; with "packed" the loader carries the rows' item counts
(host_windows=True: the same tensors in the same order) and `model.recommend_items` searches on the valid tokens only,
returning the padded run's items and scores (configs/decoder_amazon_recommend_packed.gin).
"""
import torch

from data.processed import ItemData, RecDataset, SeqData
from data.seq_loader import TokenizedSeqLoader
from evaluate.metrics import TopKAccumulator
from modules.model import EncoderDecoderRetrievalModel
from modules.tokenizer.semids import SemanticIdTokenizer
from modules.utils import parse_config
from rqhip import ops
from train_decoder import encoder_rows, load_checkpoint

try:
    import gin
except ImportError:  # pragma: no cover
    from rqhip import ginlite as gin


@gin.configurable
def recommend(
    checkpoint_path=None,
    batch_size=64,
    dataset_folder="dataset/ml-1m",
    dataset=RecDataset.ML_1M,
    pretrained_rqvae_path=None,
    force_dataset_process=False,
    vae_input_dim=18,
    vae_embed_dim=16,
    vae_hidden_dims=[18, 18],
    vae_codebook_size=32,
    vae_codebook_normalize=False,
    vae_sim_vq=False,
    vae_n_cat_feats=18,
    vae_n_layers=3,
    dataset_split="beauty",
    t5_d_model=128,
    t5_num_heads=6,
    t5_d_ff=1024,
    t5_num_layers=4,
    top_k_for_generation=10,
    should_add_sep_token=True,
    num_user_bins=None,
    top_k_eval_list=[1, 5, 10],
    beam_impl="exact",
    attention_impl="hip",
    norm_impl="hip",
    ffn_impl="hip",
    embed_impl="hip",
    max_batches=None,
    n_items=10,
    exclude_history=True,
    output_path=None,
):
    rows = encoder_rows()      # "padded", or "packed" by the binding encoder_rows.mode: validated before any other work
    if checkpoint_path is None:
        raise ValueError("recommend needs checkpoint_path: a checkpoint written by train_decoder.py")
    if dataset != RecDataset.AMAZON:
        raise Exception(f"Dataset currently not supported: {dataset}.")
    if not torch.cuda.is_available():
        raise RuntimeError("recommend needs a ROCm GPU: the batches, the beam search and the item expansion are HIP kernels")
    device = torch.device("cuda", torch.cuda.current_device())

    item_dataset = ItemData(root=dataset_folder, dataset=dataset, force_process=force_dataset_process,
                            split=dataset_split).to_device(device)
    eval_dataset = SeqData(root=dataset_folder, dataset=dataset, is_train=False, subsample=False,
                           split=dataset_split).to_device(device)

    tokenizer = SemanticIdTokenizer(
        input_dim=vae_input_dim, hidden_dims=vae_hidden_dims, output_dim=vae_embed_dim, codebook_size=vae_codebook_size,
        n_layers=vae_n_layers, n_cat_feats=vae_n_cat_feats, rqvae_weights_path=pretrained_rqvae_path,
        rqvae_codebook_normalize=vae_codebook_normalize, rqvae_sim_vq=vae_sim_vq).to(device)
    tokenizer.precompute_corpus_ids(item_dataset)
    corpus = tokenizer.cached_ids[:, :vae_n_layers].contiguous()
    # packed: the batches carry their rows' item counts on the host; same tensors, same order (no shuffle, no subsampling)
    eval_dataloader = TokenizedSeqLoader(eval_dataset, tokenizer, batch_size, shuffle=False, host_windows=rows == "packed")

    model = EncoderDecoderRetrievalModel(
        codebooks=torch.zeros_like(corpus), num_hierarchies=vae_n_layers, num_embeddings_per_hierarchy=vae_codebook_size,
        t5_d_model=t5_d_model, t5_num_heads=t5_num_heads, t5_d_ff=t5_d_ff, t5_num_layers=t5_num_layers,
        top_k_for_generation=top_k_for_generation, should_add_sep_token=should_add_sep_token,
        num_user_bins=num_user_bins).to(device)
    load_checkpoint(checkpoint_path, model, map_location=device)
    if not torch.equal(model.codebooks, corpus):
        raise ValueError(
            f"{checkpoint_path}: the tokenizer's corpus ids differ from the checkpoint's `codebooks` buffer -- the model "
            "would search another corpus than the one it was trained on; pass the RQ-VAE the decoder was trained with "
            "(pretrained_rqvae_path) and the same dataset")
    model.attention_impl, model.norm_impl, model.ffn_impl, model.embed_impl = attention_impl, norm_impl, ffn_impl, embed_impl
    model.beam_impl = beam_impl
    model.encoder_rows = rows
    model.eval()

    item_metrics = TopKAccumulator(ks=top_k_eval_list)
    sid_metrics = TopKAccumulator(ks=top_k_eval_list)
    item_index = model._item_index_for_codebooks()
    users = 0
    bad_targets = torch.zeros((), dtype=torch.int64, device=device)      # targets that are no corpus row
    in_history = torch.zeros((), dtype=torch.int64, device=device)       # users whose target is one of their history items
    all_items, all_scores = [], []
    for n, tokenized_data in enumerate(eval_dataloader):
        if max_batches is not None and n >= max_batches:
            break
        rec = model.recommend_items(tokenized_data, n_items=n_items, exclude_history=exclude_history)
        target = tokenized_data.sem_ids_fut[:, :vae_n_layers + 1]
        target_item = item_index.items_of(target)
        bad_targets += (target_item < 0).sum()
        item_metrics.accumulate(actual=target_item[:, None], top_k=rec.items[:, :, None].contiguous())
        sid_metrics.accumulate(actual=tokenized_data.sem_ids_fut[:, :vae_n_layers], top_k=rec.sem_ids)
        B = target.shape[0]
        history = tokenized_data.sem_ids.reshape(B, -1, vae_n_layers + 1)
        in_history += (ops.topk_first_match(target.contiguous(), history.contiguous()) >= 0).sum()
        users += B
        if output_path is not None:
            all_items.append(rec.items)
            all_scores.append(rec.scores)
    if users == 0:
        raise ValueError("recommend: the eval split gave no batch (max_batches=0 or an empty split)")
    counts = torch.stack([bad_targets, in_history]).tolist()              # the one host read, with reduce() below
    if counts[0] != 0:
        raise ValueError(f"recommend: {counts[0]} of {users} targets are no corpus row (tuple, dedup rank): the item-level "
                         "metrics are undefined for them")
    result = {"item": item_metrics.reduce(), "sid": sid_metrics.reduce(), "users": users, "targets_in_history": counts[1]}
    if output_path is not None:
        torch.save({"items": torch.cat(all_items).cpu(), "scores": torch.cat(all_scores).cpu()}, output_path)
    print(result)
    return result


if __name__ == "__main__":
    parse_config()
    recommend()
