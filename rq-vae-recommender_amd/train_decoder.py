"""`python train_decoder.py <config.gin>` -- training of the generative retrieval model on MI355X.

The reference's entry point (train_decoder.py) for this project: the same gin-configurable `train(...)` with every
parameter name and default of the reference, the same schedule (gradient accumulation, optimizer and scheduler step,
partial eval, full eval with beam search, checkpoint cadence) and the same checkpoint dictionary (`iter`, `model`,
`optimizer`, `scheduler`; state-dict keys unchanged, so a reference checkpoint resumes here: the `_orig_mod.` prefix
its compiled model writes is accepted on load).

What differs:
  * one process, one GPU: no accelerate, no torch.compile.  `split_batches` is accepted and unused.
  * the input path.  The histories live on the device in CSR form (data/processed.py:SeqData.to_device) and a batch --
    semantic ids, mask, target, user ids -- is ONE kernel launch behind one `torch.randint`
    (data/seq_loader.py:TokenizedSeqLoader, csrc/seq_batch.hip) instead of a Python `__getitem__` per user, a collate,
    a copy and `SemanticIdTokenizer.forward`.  Windows follow the reference's law on torch's device generator, not
    Python's `random`: same distribution, another sample sequence.  The range test the reference makes per batch
    (`ids.max()`, a host stall) is made once, when the loaders are built.
  * the model's fused paths, chosen by five extra parameters: attention_impl ("hip_train"), norm_impl, ffn_impl,
    head_impl, embed_impl ("hip"); "torch" selects the operators.  Each falls back to the operators silently where its
    kernel does not implement the shape (modules/model.py, modules/t5.py).
  * clip, schedule and AdamW run on the device (rqhip/optim.py:FlatAdamW with the InverseSquareRootScheduler attached);
    the loss is read back every `log_every` iterations only, next to `optimizer.grad_norm` and `optimizer.device_lr()`.
  * amp=True with mixed_precision_type="bf16" sets `model.matmul_arith = "bf16"` (modules/t5.py): the matrix products
    of the "hip" feed-forward, and of the "hip" projections where `model.proj_impl` selects them (train has no parameter
    for it: the model's default is "torch"), take bf16 operands and accumulate in fp32.  There is no autocast: weights,
    activations, gradients, the checkpoint, the attention, the norms, the heads, the embedding and the optimizer stay
    fp32, and the "torch" bodies are not affected.  amp=True with any other type raises: those kernels are fp32 or
    bf16-operand only.  The bf16 arm of the long attention calls is `model.attention_arith = "bf16"` (modules/t5.py),
    an attribute set on the model: train has no parameter for it, nor for `model.attention_long_impl`, and amp does
    not set it.  Reading the bf16 arm's weights from bf16 images, `model.weight_images = "bf16"` (modules/t5.py), is
    a model attribute of the same kind: no parameter here, and amp goes on setting `matmul_arith` alone; the images
    follow every FlatAdamW step through rqhip.optim.generation().  So is `model.saved_activations = "bf16"`
    (modules/t5.py), which makes the bf16 feed-forward keep bf16 images of its activations for the backward.
  * packed encoder rows.  `encoder_rows` below is a gin-configurable of its own, not a parameter of `train`, whose
    parameter set stays the reference's plus the six kernel and logging choices (tests/test_seq_batch_host.py pins it).
    The binding `encoder_rows.mode = "packed"` (default "padded"; a config line, or gin.parse_config from Python) makes
    `train` set `model.encoder_rows` (modules/model.py) and build both loaders with host_windows=True (data/seq_loader.py): the windows are drawn on the host, every batch says how many items each row
    holds, and the encoder, the cross-attention K/V and every kernel between them run on the valid tokens only.  The
    number of rows of such a step depends on the data, so a packed step cannot be captured into a graph.  The
    checkpoint is the same: it loads into a padded model and back.  configs/decoder_amazon_packed.gin.
    The binding covers the training steps and the partial evals.  The full eval's beam search stays PADDED in this
    script, although its batches carry their counts and `model.generate_next_sem_id` would run them packed with the
    same bits (modules/model.py): tests/test_gpu_packed_model.py pins the packed and pack calls of a packed training
    run that ends in a full eval, and that pin is kept.  evaluate_decoder.py and recommend.py read the same binding
    and run the search packed (configs/decoder_amazon_eval_packed.gin, configs/decoder_amazon_recommend_packed.gin).
    push_vae_to_hf=True raises: it needs the network.  Datasets other than AMAZON raise, as in the
    reference.
wandb is optional: with `wandb_logging=True` and no wandb module, metrics are printed.
The full eval here reports one draw of the sampling beam search; evaluate_decoder.py evaluates a checkpoint with the
exact constrained search (`model.beam_impl = "exact"`), whose metrics do not depend on the seed.

Not done: replaying the step from a captured hipGraph (the loader's calls make no host read and no data-dependent
allocation, so they can be recorded), and training on several ranks.
"""
import os
import time

import torch

from data.processed import ItemData, RecDataset, SeqData
from data.seq_loader import TokenizedSeqLoader
from data.utils import cycle
from evaluate.metrics import TopKAccumulator
from modules.model import ENCODER_ROWS, EncoderDecoderRetrievalModel
from modules.scheduler.inv_sqrt import InverseSquareRootScheduler
from modules.tokenizer.semids import SemanticIdTokenizer
from modules.utils import parse_config
from rqhip.optim import FlatAdamW

try:
    import gin
except ImportError:  # pragma: no cover
    from rqhip import ginlite as gin

try:
    import wandb  # noqa: F401
    _HAVE_WANDB = True
except ImportError:  # pragma: no cover
    wandb = None
    _HAVE_WANDB = False

COMPILE_PREFIX = "_orig_mod."


def strip_compile_prefix(state_dict: dict) -> dict:
    """A model state dict with the `_orig_mod.` prefix of a torch.compile'd module removed from every key that has it
    (the reference saves its compiled model); other keys are kept as they are."""
    return {(k[len(COMPILE_PREFIX):] if k.startswith(COMPILE_PREFIX) else k): v for k, v in state_dict.items()}


def load_checkpoint(path: str, model, optimizer=None, lr_scheduler=None, map_location=None) -> int:
    """Load a `{"iter", "model", "optimizer", "scheduler"}` checkpoint -> the iteration to continue from (iter + 1)."""
    state = torch.load(path, map_location=map_location, weights_only=False)
    model.load_state_dict(strip_compile_prefix(state["model"]))
    if optimizer is not None:
        optimizer.load_state_dict(state["optimizer"])
    if lr_scheduler is not None and "scheduler" in state:
        lr_scheduler.load_state_dict(state["scheduler"])
    return state["iter"] + 1


@gin.configurable
def encoder_rows(mode="padded"):
    """How `train` lays out the encoder's rows (module docstring): "padded", or "packed" -- bound as
    `encoder_rows.mode = "packed"`, which configs/decoder_amazon_packed.gin adds to configs/decoder_amazon.gin."""
    if mode not in ENCODER_ROWS:
        raise ValueError(f"encoder_rows.mode must be one of {ENCODER_ROWS}, got {mode!r}")
    return mode


@gin.configurable
def train(
    iterations=500000,
    batch_size=64,
    learning_rate=0.001,
    weight_decay=0.01,
    dataset_folder="dataset/ml-1m",
    save_dir_root="out/",
    dataset=RecDataset.ML_1M,
    pretrained_rqvae_path=None,
    pretrained_decoder_path=None,
    split_batches=True,
    amp=False,
    wandb_logging=False,
    force_dataset_process=False,
    mixed_precision_type="fp16",
    gradient_accumulate_every=1,
    save_model_every=1000000,
    partial_eval_every=1000,
    full_eval_every=10000,
    vae_input_dim=18,
    vae_embed_dim=16,
    vae_hidden_dims=[18, 18],
    vae_codebook_size=32,
    vae_codebook_normalize=False,
    vae_sim_vq=False,
    vae_n_cat_feats=18,
    vae_n_layers=3,
    dataset_split="beauty",
    push_vae_to_hf=False,
    train_data_subsample=True,
    vae_hf_model_name="edobotta/rqvae-amazon-beauty",
    max_grad_norm=None,
    t5_d_model=128,
    t5_num_heads=6,
    t5_d_ff=1024,
    t5_num_layers=4,
    top_k_for_generation=10,
    should_add_sep_token=True,
    num_user_bins=None,
    top_k_eval_list=[1, 5, 10],
    attention_impl="hip_train",
    norm_impl="hip",
    ffn_impl="hip",
    head_impl="hip",
    embed_impl="hip",
    log_every=100,
):
    params = dict(locals())
    del split_batches, vae_hf_model_name
    if dataset != RecDataset.AMAZON:
        raise Exception(f"Dataset currently not supported: {dataset}.")
    if amp and mixed_precision_type != "bf16":
        raise NotImplementedError(
            f"amp=True ({mixed_precision_type}): the fused T5 kernels (attention, add/norm, heads, embedding) and the "
            'device optimizer are fp32 only; the feed-forward and projection kernels are fp32 or, with '
            'mixed_precision_type="bf16", bf16-operand')
    rows = encoder_rows()      # "padded", or "packed" by the binding encoder_rows.mode (validated there)
    if push_vae_to_hf:
        raise NotImplementedError("push_vae_to_hf=True needs the network (huggingface_hub); upload the RQ-VAE checkpoint "
                                  "separately")
    if not torch.cuda.is_available():
        raise RuntimeError("train_decoder needs a ROCm GPU: the batches, the beam search and the optimizer are HIP kernels")
    device = torch.device("cuda", torch.cuda.current_device())

    use_wandb = wandb_logging and _HAVE_WANDB
    if wandb_logging and not _HAVE_WANDB:
        print("wandb is not installed: metrics go to stdout")
    if use_wandb:
        wandb.login()
        wandb.init(project="gen-retrieval-decoder-training", config=params)

    def emit(log: dict) -> None:
        if use_wandb:
            wandb.log(log)
        elif wandb_logging:
            print({k: (round(v, 6) if isinstance(v, float) else v) for k, v in log.items()})

    item_dataset = ItemData(root=dataset_folder, dataset=dataset, force_process=force_dataset_process,
                            split=dataset_split).to_device(device)
    train_dataset = SeqData(root=dataset_folder, dataset=dataset, is_train=True, subsample=train_data_subsample,
                            split=dataset_split).to_device(device)
    eval_dataset = SeqData(root=dataset_folder, dataset=dataset, is_train=False, subsample=False,
                           split=dataset_split).to_device(device)

    tokenizer = SemanticIdTokenizer(
        input_dim=vae_input_dim, hidden_dims=vae_hidden_dims, output_dim=vae_embed_dim, codebook_size=vae_codebook_size,
        n_layers=vae_n_layers, n_cat_feats=vae_n_cat_feats, rqvae_weights_path=pretrained_rqvae_path,
        rqvae_codebook_normalize=vae_codebook_normalize, rqvae_sim_vq=vae_sim_vq).to(device)
    tokenizer.precompute_corpus_ids(item_dataset)

    # (the loaders check every stored item id against the corpus once, here)
    host_windows = rows == "packed"    # the batches then carry their rows' item counts on the host
    train_dataloader = cycle(TokenizedSeqLoader(train_dataset, tokenizer, batch_size, shuffle=True,
                                                host_windows=host_windows))
    eval_dataloader = TokenizedSeqLoader(eval_dataset, tokenizer, batch_size, shuffle=True, host_windows=host_windows)

    model = EncoderDecoderRetrievalModel(
        codebooks=tokenizer.cached_ids[:, :vae_n_layers].contiguous(), num_hierarchies=vae_n_layers,
        num_embeddings_per_hierarchy=vae_codebook_size, t5_d_model=t5_d_model, t5_num_heads=t5_num_heads, t5_d_ff=t5_d_ff,
        t5_num_layers=t5_num_layers, top_k_for_generation=top_k_for_generation, should_add_sep_token=should_add_sep_token,
        num_user_bins=num_user_bins).to(device)
    model.attention_impl, model.norm_impl, model.ffn_impl = attention_impl, norm_impl, ffn_impl
    model.head_impl, model.embed_impl = head_impl, embed_impl
    model.encoder_rows = rows
    if amp:
        model.matmul_arith = "bf16"

    optimizer = FlatAdamW(model.parameters(), lr=learning_rate, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
    lr_scheduler = InverseSquareRootScheduler(optimizer=optimizer, warmup_steps=10000)

    start_iter = 0
    if pretrained_decoder_path is not None:
        start_iter = load_checkpoint(pretrained_decoder_path, model, optimizer, lr_scheduler, map_location=device)

    metrics_accumulator = TopKAccumulator(ks=top_k_eval_list)
    num_params = sum(p.numel() for p in model.parameters())
    print(f"Device: {device}, Num Parameters: {num_params}")

    losses, eval_losses, eval_metrics, checkpoint_path = [], [], {}, None
    end_iter = start_iter + iterations
    t0 = time.time()
    for it in range(start_iter, end_iter):
        model.train()
        total_loss = None
        optimizer.zero_grad()
        for _ in range(gradient_accumulate_every):
            tokenized_data = next(train_dataloader)
            loss = model(tokenized_data).loss / gradient_accumulate_every
            loss.backward()
            total_loss = loss.detach() if total_loss is None else total_loss + loss.detach()
        assert model.item_sid_embedding_table.weight.grad is not None

        optimizer.step()
        lr_scheduler.step()

        if (it + 1) % log_every == 0:
            # the step's only host reads: the loss, the gradient norm before clipping (NaN without clipping) and the lr
            shown = torch.stack([total_loss, optimizer.grad_norm, optimizer.device_lr()]).tolist()
            losses.append((it, shown[0]))
            rate = (it - start_iter + 1) / max(time.time() - t0, 1e-9)
            print(f"iter {it}: loss: {shown[0]:.4f}, grad norm: {shown[1]:.4f}, lr: {shown[2]:.3e} ({rate:.1f} it/s)")
            emit({"learning_rate": shown[2], "total_loss": shown[0], "grad_norm": shown[1]})

        if (it + 1) % partial_eval_every == 0:
            model.eval()
            rows = []
            with torch.no_grad():
                for tokenized_data in eval_dataloader:
                    rows.append(model(tokenized_data).loss)
            if rows:
                eval_losses.append((it, torch.stack(rows).mean().item()))
                emit({"eval_loss": eval_losses[-1][1]})

        if (it + 1) % full_eval_every == 0:
            model.eval()
            model.encoder_rows = "padded"      # the full eval's search stays padded (module docstring)
            for tokenized_data in eval_dataloader:
                generated = model.generate_next_sem_id(tokenized_data, top_k=True, temperature=1)
                metrics_accumulator.accumulate(actual=tokenized_data.sem_ids_fut[:, :vae_n_layers], top_k=generated.sem_ids)
            model.encoder_rows = encoder_rows()
            eval_metrics = metrics_accumulator.reduce()
            print(eval_metrics)
            emit(eval_metrics)
            metrics_accumulator.reset()

        if (it + 1) % save_model_every == 0 or it + 1 == end_iter:
            state = {"iter": it, "model": model.state_dict(), "optimizer": optimizer.state_dict(),
                     "scheduler": lr_scheduler.state_dict()}
            if train_dataset.synthetic:
                state["data"] = "synthetic"   # extra key: a checkpoint trained on noise says so
            os.makedirs(save_dir_root, exist_ok=True)
            checkpoint_path = save_dir_root + f"checkpoint_{it}.pt"
            torch.save(state, checkpoint_path)

    if use_wandb:
        wandb.finish()
    return {"losses": losses, "eval_losses": eval_losses, "eval_metrics": eval_metrics, "checkpoint": checkpoint_path,
            "start_iter": start_iter, "end_iter": end_iter,
            "learning_rate": float(optimizer.device_lr()) if iterations > 0 else None}


if __name__ == "__main__":
    parse_config()
    train()
