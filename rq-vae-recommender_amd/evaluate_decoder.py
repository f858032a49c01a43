"""`python evaluate_decoder.py <config.gin>` -- retrieval metrics of one train_decoder.py checkpoint on the eval split.

An interface, not a second training script: the gin-configurable `evaluate(...)` takes the data, tokenizer, T5 and
`top_k_*` parameters of train_decoder.train under the same names and defaults, builds the item set, the eval split and
the tokenizer as `train` does, loads the checkpoint with train_decoder.load_checkpoint, runs the eval split ONCE in a
fixed order (TokenizedSeqLoader, shuffle=False) through `model.generate_next_sem_id` and returns
`TopKAccumulator.reduce()` (`ndcg`, `h@k`) plus `users`.  One process, one GPU; the metrics are printed.

`beam_impl` chooses the search (modules/model.py).  "exact", the default here, is the deterministic constrained beam
search: at every level every corpus-valid child of every kept beam is scored by its log-softmax value, the k best are
kept, equal scores (-inf included) go to the lower candidate number beam * K + code, and no random number is drawn -- so
the metrics of a checkpoint do not depend on the seed and two checkpoints can be compared from one run each.  It needs
top_k_for_generation <= vae_codebook_size (K <= 4096, k <= 64); a beam it reports as -inf means that fewer than k corpus
items share the kept prefixes, never a beam lost to chance.  "sample" is the reference's sampling search, the one the
full eval of train_decoder.train reports: its metrics are one draw.

The tokenizer must give the corpus the checkpoint was trained on: `evaluate` raises when the tokenizer's corpus ids
differ from the checkpoint's `codebooks` buffer, because the model would then search another corpus than the one the
targets come from.  The fused paths are chosen as in `train`: attention_impl ("hip", the inference kernel with slab
K/V), norm_impl, ffn_impl, embed_impl; "torch" selects the operators.  `max_batches` stops after that many batches.

Packed encoder rows: `evaluate` reads the binding `encoder_rows.mode` of train_decoder.encoder_rows (the one configurable;
"padded" by default, validated before any other work).  With "packed" it sets `model.encoder_rows` and builds its loader
with host_windows=True -- without shuffling and subsampling the same tensors in the same order, each batch also saying
how many items its rows hold -- and every search runs the encoder, the cross-attention K/V and the decode steps'
cross-attention on the valid tokens only, with the padded run's metrics (modules/model.py;
configs/decoder_amazon_eval_packed.gin; profiles/packed_generate.txt).
"""
import torch

from data.processed import ItemData, RecDataset, SeqData
from data.seq_loader import TokenizedSeqLoader
from evaluate.metrics import TopKAccumulator
from modules.model import EncoderDecoderRetrievalModel
from modules.tokenizer.semids import SemanticIdTokenizer
from modules.utils import parse_config
from train_decoder import encoder_rows, load_checkpoint

try:
    import gin
except ImportError:  # pragma: no cover
    from rqhip import ginlite as gin


@gin.configurable
def evaluate(
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
):
    rows = encoder_rows()      # "padded", or "packed" by the binding encoder_rows.mode: validated before any other work
    if checkpoint_path is None:
        raise ValueError("evaluate needs checkpoint_path: a checkpoint written by train_decoder.py")
    if dataset != RecDataset.AMAZON:
        raise Exception(f"Dataset currently not supported: {dataset}.")
    if not torch.cuda.is_available():
        raise RuntimeError("evaluate_decoder needs a ROCm GPU: the batches and the beam search are HIP kernels")
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

    metrics_accumulator = TopKAccumulator(ks=top_k_eval_list)
    users = 0
    for n, tokenized_data in enumerate(eval_dataloader):
        if max_batches is not None and n >= max_batches:
            break
        generated = model.generate_next_sem_id(tokenized_data, top_k=True, temperature=1)
        metrics_accumulator.accumulate(actual=tokenized_data.sem_ids_fut[:, :vae_n_layers], top_k=generated.sem_ids)
        users += tokenized_data.sem_ids_fut.shape[0]
    if users == 0:
        raise ValueError("evaluate: the eval split gave no batch (max_batches=0 or an empty split)")
    metrics = dict(metrics_accumulator.reduce(), users=users)
    print(metrics)
    return metrics


if __name__ == "__main__":
    parse_config()
    evaluate()
