#!/usr/bin/env python3
"""Time one training step of the retrieval model (forward + backward + AdamW, train mode, dropout 0.1) at the Amazon
decoder config (d_model 384, 6 heads, d_ff 1024, 4 layers, K = 256, L = 3; batch 64, 20-item histories with padded
tails: encoder T = 81, decoder T = 4) in fourteen arms:

  torch      the T5 operators: per attention two batched matmuls, the adds, an fp32 softmax, a dropout mask and the
             head transposes, with the [R, H, Tq, Tk] weights saved for autograd
  hip_train  one ops.t5_attention_fwd_train launch per attention and one ops.t5_attention_bwd launch in the backward
  hip_train+norm  hip_train with norm_impl = "hip": each dropout + residual add + RMS norm between two sub-layer bodies
             as one ops.t5_add_norm_fwd launch and one ops.t5_add_norm_bwd call
  hip_train+norm+head  hip_train+norm with head_impl = "hip": the three heads and their cross-entropy losses as one
             ops.sid_head_loss_fwd call and one ops.sid_head_loss_bwd launch
  hip_train+norm+head+ffn  hip_train+norm+head with ffn_impl = "hip": each feed-forward body (wi, ReLU, dropout, wo) as
             one ops.t5_ffn_fwd launch and one ops.t5_ffn_bwd call of two launches
  hip_train+norm+head+ffn+optim  hip_train+norm+head+ffn stepped by rqhip.optim.FlatAdamW (csrc/adamw.hip: one bump launch and
             one update launch per 24 tensors) instead of torch.optim.AdamW; no clipping and no schedule, as in the other arms
  hip_train+norm+head+ffn+optim+embed  the arm before it with embed_impl = "hip": each stack's input embedding (offsets,
             mask product, gather, separator, BOS row) as one ops.sid_embed_fwd launch and one ops.sid_embed_bwd launch
  hip_train+norm+head+ffn+optim+embed+proj  the arm before it with proj_impl = "hip": the q / k / v, the o and the
             cross-attention K/V projections as grouped ops.t5_proj_fwd launches and ops.t5_proj_bwd calls of two launches
  hip_train+norm+head+ffn+optim+embed+bf16  the seventh arm with matmul_arith = "bf16": the feed-forward's matrix
             products on bf16 operands with fp32 accumulation (rqhip_t5_ffn_*_bf16), everything stored in fp32
  hip_train+norm+head+ffn+optim+embed+proj+bf16  the eighth arm with matmul_arith = "bf16": the feed-forward and the
             grouped projections on bf16 operands (rqhip_t5_ffn_*_bf16, rqhip_t5_proj_*_bf16)
  ...+bf16+img  either bf16 arm with weight_images = "bf16": the same products with the weights read from bf16 images
             (rqhip_t5_ffn_*_bf16w, rqhip_t5_proj_*_bf16w), refreshed by one launch per stack and step; the same bits
  ...+bf16+img+act  either +img arm with saved_activations = "bf16": the feed-forward saves blocked bf16 images of its
             two activations in place of fp32 tensors and its backward reads them (rqhip_t5_ffn_*_bf16wa); the same bits

  <arm>+packed  any arm above with model.encoder_rows = "packed" (modules/model.py): the batch carries its rows' item
             counts (data.schemas.CountedSeqBatch) and the encoder, the cross-attention K/V and every kernel between them
             run on the valid tokens only (ops.rows_pack, ops.t5_attention_packed*); without a fused attention it is the
             arm itself
--data picks the batches every arm steps through, the same ones in the same order: "tails" (the default: one batch, the
last b % 20 items of row b padded), "full" (one batch, every history full: fill 1.0) or "loader" (--batches batches drawn
once from data.seq_loader.TokenizedSeqLoader over the synthetic:12101 histories under the training window law, cycled).
The summary reports their fill: valid history items over item slots.

The arms alternate --runs times in one process on one device (same weights at the start of every block, same
batch); each block is --warmup untimed steps, then --iters steps with a device event pair around each.  Reports the
median and the fastest step per arm over all blocks, the median of each block (their spread is what a difference
between two arms has to exceed), and the peak torch.cuda.max_memory_allocated of a block, as one
JSON line per arm plus a summary line; --out also writes them to a text file (profiles/retrieval_train_step_norm.txt
holds a three-arm run, profiles/retrieval_train_step_head.txt a four-arm run, profiles/retrieval_train_step_ffn.txt a
five-arm run, profiles/retrieval_optim_tail.txt a six-arm run, profiles/retrieval_train_step_embed.txt a run of the sixth
and seventh arm, profiles/retrieval_train_step_proj.txt runs of the seventh and eighth,
profiles/retrieval_train_step_bf16.txt runs of those two and their bf16 forms, profiles/t5_weight_images.txt runs of
the bf16 forms with and without +img, profiles/t5_saved_activations.txt runs of the +img forms with and without +act;
profiles/retrieval_train_step.txt is the
older two-arm run; none of them is to be overwritten or compared
against: two arms are compared within one run only).
--arms picks a subset, e.g. one arm under a kernel trace to count its launches per step.

    python tools/bench_retrieval_train.py [--runs 5] [--warmup 3] [--iters 10] [--batch 64] [--arms A,B] [--out FILE]
                                          [--data tails|full|loader] [--batches 8]
"""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rq-vae-recommender_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402

from modules.model import EncoderDecoderRetrievalModel  # noqa: E402
from retrieval_cases import synthetic_batch, to_device  # noqa: E402  (tests/retrieval_cases.py)

# arm -> (attention_impl, norm_impl, head_impl, ffn_impl, proj_impl)
ARMS = {"torch": ("torch", "torch", "torch", "torch", "torch"),
        "hip_train": ("hip_train", "torch", "torch", "torch", "torch"),
        "hip_train+norm": ("hip_train", "hip", "torch", "torch", "torch"),
        "hip_train+norm+head": ("hip_train", "hip", "hip", "torch", "torch"),
        "hip_train+norm+head+ffn": ("hip_train", "hip", "hip", "hip", "torch"),
        "hip_train+norm+head+ffn+optim": ("hip_train", "hip", "hip", "hip", "torch"),
        "hip_train+norm+head+ffn+optim+embed": ("hip_train", "hip", "hip", "hip", "torch"),
        "hip_train+norm+head+ffn+optim+embed+proj": ("hip_train", "hip", "hip", "hip", "hip"),
        "hip_train+norm+head+ffn+optim+embed+bf16": ("hip_train", "hip", "hip", "hip", "torch"),
        "hip_train+norm+head+ffn+optim+embed+proj+bf16": ("hip_train", "hip", "hip", "hip", "hip"),
        "hip_train+norm+head+ffn+optim+embed+bf16+img": ("hip_train", "hip", "hip", "hip", "torch"),
        "hip_train+norm+head+ffn+optim+embed+proj+bf16+img": ("hip_train", "hip", "hip", "hip", "hip"),
        "hip_train+norm+head+ffn+optim+embed+bf16+img+act": ("hip_train", "hip", "hip", "hip", "torch"),
        "hip_train+norm+head+ffn+optim+embed+proj+bf16+img+act": ("hip_train", "hip", "hip", "hip", "hip")}
# arms with saved_activations = "bf16"; the others "fp32"
ACT = ("hip_train+norm+head+ffn+optim+embed+bf16+img+act", "hip_train+norm+head+ffn+optim+embed+proj+bf16+img+act")
# arms with weight_images = "bf16"; the others "none"
IMG = ("hip_train+norm+head+ffn+optim+embed+bf16+img", "hip_train+norm+head+ffn+optim+embed+proj+bf16+img") + ACT
# arms with matmul_arith = "bf16"; the others "fp32"
BF16 = ("hip_train+norm+head+ffn+optim+embed+bf16", "hip_train+norm+head+ffn+optim+embed+proj+bf16") + IMG
# arms stepped by rqhip.optim.FlatAdamW; the others by torch.optim.AdamW
FLAT_ADAMW = ("hip_train+norm+head+ffn+optim", "hip_train+norm+head+ffn+optim+embed",
              "hip_train+norm+head+ffn+optim+embed+proj") + BF16
# arms with embed_impl = "hip"; the others "torch"
EMBED_HIP = ("hip_train+norm+head+ffn+optim+embed", "hip_train+norm+head+ffn+optim+embed+proj") + BF16


PACKED = "+packed"


def base_arm(arm):
    return arm[:-len(PACKED)] if arm.endswith(PACKED) else arm


def counted(batch, L):
    """The batch as a CountedSeqBatch, the rows' item counts read from its own mask (once, before any timing)."""
    from data.schemas import CountedSeqBatch
    counts = batch.seq_mask.view(batch.seq_mask.shape[0], -1, L + 1)[:, :, 0].sum(1).cpu().to(torch.int64)
    return CountedSeqBatch(*batch, item_counts=counts)


def make_batch(B, items, L, K, N, dev, seed, pad="b_mod_items"):
    g = torch.Generator().manual_seed(seed)
    corpus = torch.randint(0, K, (N, L), generator=g)
    return corpus, counted(to_device(synthetic_batch(corpus, B, items, g, pad=pad), dev), L)


def loader_batches(corpus, B, n, dev, seed):
    """n training batches of B rows from TokenizedSeqLoader(host_windows=True) over the synthetic histories of the
    corpus' size, under the training window law (subsample)."""
    from data.processed import RecDataset, SeqData
    from data.seq_loader import TokenizedSeqLoader
    from modules.tokenizer.semids import SemanticIdTokenizer
    N, L = corpus.shape
    ds = SeqData(root=f"synthetic:{N}", dataset=RecDataset.AMAZON, is_train=True, subsample=True).to_device(dev)
    tok = SemanticIdTokenizer(input_dim=16, output_dim=8, hidden_dims=[16], codebook_size=256, n_layers=L, n_cat_feats=0)
    tok.cached_ids = torch.cat([corpus, torch.zeros(N, 1, dtype=torch.long)], dim=1).to(dev)
    torch.manual_seed(seed)
    out = []
    for batch in TokenizedSeqLoader(ds, tok, B, shuffle=True, host_windows=True):
        if batch.sem_ids.shape[0] == B:
            out.append(batch)
        if len(out) == n:
            break
    return out


def block(model, state, batches, arm, warmup, iters):
    """One block of one arm from the common starting weights -> (ms per step, peak bytes, last loss)."""
    model.load_state_dict(state)
    model.encoder_rows = "packed" if arm.endswith(PACKED) else "padded"
    arm = base_arm(arm)
    model.attention_impl, model.norm_impl, model.head_impl, model.ffn_impl, model.proj_impl = ARMS[arm]
    model.embed_impl = "hip" if arm in EMBED_HIP else "torch"
    model.matmul_arith = "bf16" if arm in BF16 else "fp32"
    model.weight_images = "bf16" if arm in IMG else "none"
    model.saved_activations = "bf16" if arm in ACT else "fp32"
    model.train()
    if arm in FLAT_ADAMW:
        from rqhip.optim import FlatAdamW
        opt = FlatAdamW(model.parameters(), lr=1e-3)
    else:
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    torch.manual_seed(0)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for it in range(warmup + iters):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        opt.zero_grad()
        out = model(batches[it % len(batches)])
        out.loss.backward()
        opt.step()
        stop.record()
        stop.synchronize()
        if it >= warmup:
            ms.append(start.elapsed_time(stop))
    return ms, torch.cuda.max_memory_allocated(), out.loss.item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--arms", default=",".join(ARMS), help="comma-separated subset of: " + ", ".join(ARMS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--data", default="tails", choices=("tails", "full", "loader"))
    ap.add_argument("--batches", type=int, default=8, help="batches drawn with --data loader")
    args = ap.parse_args()
    arms = args.arms.split(",")
    if not arms or any(base_arm(a) not in ARMS for a in arms):
        ap.error(f"--arms takes names from {list(ARMS)}, each also with the suffix {PACKED}")
    dev = torch.device("cuda")
    corpus, batch = make_batch(args.batch, 20, 3, 256, 12101, dev, 5, pad="none" if args.data == "full" else "b_mod_items")
    batches = loader_batches(corpus, args.batch, args.batches, dev, 5) if args.data == "loader" else [batch]
    fill = sum(float(b.item_counts.float().mean()) for b in batches) / len(batches) / 20
    rows = sum(int(b.item_counts.sum()) * 4 for b in batches) / len(batches)
    torch.manual_seed(5)
    model = EncoderDecoderRetrievalModel(corpus, 3, 256, t5_d_model=384, t5_num_heads=6, t5_d_ff=1024,
                                         t5_num_layers=4).to(dev)
    state = copy.deepcopy(model.state_dict())
    times = {a: [] for a in arms}
    peak = {a: 0 for a in arms}
    blocks = {a: [] for a in arms}
    loss = {}
    for _ in range(args.runs):
        for arm in arms:
            ms, mem, loss[arm] = block(model, state, batches, arm, args.warmup, args.iters)
            times[arm] += ms
            blocks[arm].append(round(statistics.median(ms), 3))
            peak[arm] = max(peak[arm], mem)
    lines = []
    for name in arms:
        arm = base_arm(name)
        lines.append(json.dumps({"arm": name, "attention_impl": ARMS[arm][0], "norm_impl": ARMS[arm][1],
                                 "head_impl": ARMS[arm][2], "ffn_impl": ARMS[arm][3], "proj_impl": ARMS[arm][4],
                                 **({"embed_impl": "hip"} if arm in EMBED_HIP else {}),
                                 **({"matmul_arith": "bf16"} if arm in BF16 else {}),
                                 **({"weight_images": "bf16"} if arm in IMG else {}),
                                 **({"saved_activations": "bf16"} if arm in ACT else {}),
                                 **({"encoder_rows": "packed"} if name.endswith(PACKED) else {}),
                                 "optimizer": "FlatAdamW" if arm in FLAT_ADAMW else "torch.optim.AdamW", "batch": args.batch,
                                 "steps_timed": len(times[name]),
                                 "ms_per_step_median": round(statistics.median(times[name]), 3),
                                 "ms_per_step_min": round(min(times[name]), 3), "block_medians": blocks[name],
                                 "peak_allocated_MiB": round(peak[name] / 2 ** 20, 1),
                                 "last_loss": round(loss[name], 4)}))
    summary = {"summary": "median step, first arm / second arm"}
    for a, b in (("torch", "hip_train"), ("hip_train", "hip_train+norm"), ("hip_train+norm", "hip_train+norm+head"),
                 ("hip_train+norm+head", "hip_train+norm+head+ffn"),
                 ("hip_train+norm+head+ffn", "hip_train+norm+head+ffn+optim"),
                 ("hip_train+norm+head+ffn+optim", "hip_train+norm+head+ffn+optim+embed"),
                 ("hip_train+norm+head+ffn+optim+embed", "hip_train+norm+head+ffn+optim+embed+proj"),
                 ("hip_train+norm+head+ffn+optim+embed", "hip_train+norm+head+ffn+optim+embed+bf16"),
                 ("hip_train+norm+head+ffn+optim+embed+proj", "hip_train+norm+head+ffn+optim+embed+proj+bf16"),
                 ("hip_train+norm+head+ffn+optim+embed+bf16", "hip_train+norm+head+ffn+optim+embed+bf16+img"),
                 ("hip_train+norm+head+ffn+optim+embed+proj+bf16", "hip_train+norm+head+ffn+optim+embed+proj+bf16+img"),
                 ("hip_train+norm+head+ffn+optim+embed+bf16+img", "hip_train+norm+head+ffn+optim+embed+bf16+img+act"),
                 ("hip_train+norm+head+ffn+optim+embed+proj+bf16+img",
                  "hip_train+norm+head+ffn+optim+embed+proj+bf16+img+act")):
        if a in arms and b in arms:
            summary[f"{a} / {b}"] = round(statistics.median(times[a]) / statistics.median(times[b]), 3)
            summary[f"peak {a} / {b}"] = round(peak[a] / peak[b], 3)
    for a in arms:      # each packed arm against its padded twin
        if a.endswith(PACKED) and base_arm(a) in arms:
            b = base_arm(a)
            summary[f"{b} / {a}"] = round(statistics.median(times[b]) / statistics.median(times[a]), 3)
            summary[f"peak {b} / {a}"] = round(peak[b] / peak[a], 3)
    summary.update({"data": args.data, "batches": len(batches), "fill": round(fill, 3),
                    "encoder_tokens_valid_per_batch": rows, "encoder_tokens_padded_per_batch": args.batch * 80})
    summary.update({"device": torch.cuda.get_device_name(0), "runs": args.runs, "warmup": args.warmup,
                    "iters": args.iters})
    lines.append(json.dumps(summary))
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
