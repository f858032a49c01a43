#!/usr/bin/env python3
"""Time one training step of the retrieval model (forward + backward + AdamW, train mode, dropout 0.1) at the Amazon
decoder config (d_model 384, 6 heads, d_ff 1024, 4 layers, K = 256, L = 3; batch 64, 20-item histories with padded
tails: encoder T = 81, decoder T = 4) with either attention implementation:

  torch      the T5 operators: per attention two batched matmuls, the adds, an fp32 softmax, a dropout mask and the
             head transposes, with the [R, H, Tq, Tk] weights saved for autograd
  hip_train  one ops.t5_attention_fwd_train launch per attention and one ops.t5_attention_bwd launch in the backward

The two arms alternate --runs times in one process on one device (same weights at the start of every block, same
batch); each block is --warmup untimed steps, then --iters steps with a device event pair around each.  Reports the
median and the fastest step per arm over all blocks, and the peak torch.cuda.max_memory_allocated of a block, as one
JSON line per arm plus a summary line; --out also writes them to a text file (profiles/retrieval_train_step.txt).

    python tools/bench_retrieval_train.py [--runs 5] [--warmup 3] [--iters 10] [--batch 64] [--out FILE]
"""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rq-vae-recommender_amd")]

import torch  # noqa: E402

from data.schemas import TokenizedSeqBatch  # noqa: E402
from modules.model import EncoderDecoderRetrievalModel  # noqa: E402

ARMS = ("torch", "hip_train")


def make_batch(B, items, L, K, N, dev, seed):
    g = torch.Generator().manual_seed(seed)
    corpus = torch.randint(0, K, (N, L), generator=g)
    hist = torch.cat([corpus[torch.randint(0, N, (B, items), generator=g)], torch.zeros(B, items, 1, dtype=torch.long)],
                     dim=-1)
    mask = torch.ones(B, items, L + 1, dtype=torch.bool)
    for b in range(B):
        pad = b % items
        if pad:
            hist[b, items - pad:] = -1
            mask[b, items - pad:] = False
    fut = torch.cat([corpus[torch.randint(0, N, (B,), generator=g)], torch.zeros(B, 1, dtype=torch.long)], dim=-1)
    batch = TokenizedSeqBatch(torch.randint(0, 100, (B, 1), generator=g), hist.reshape(B, -1), fut, mask.reshape(B, -1),
                              None, None)
    return corpus, TokenizedSeqBatch(*[None if t is None else t.to(dev) for t in batch])


def block(model, state, batch, impl, warmup, iters):
    """One block of one arm from the common starting weights -> (ms per step, peak bytes, last loss)."""
    model.load_state_dict(state)
    model.attention_impl = impl
    model.train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    torch.manual_seed(0)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for it in range(warmup + iters):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        opt.zero_grad()
        out = model(batch)
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    corpus, batch = make_batch(args.batch, 20, 3, 256, 12101, dev, 5)
    torch.manual_seed(5)
    model = EncoderDecoderRetrievalModel(corpus, 3, 256, t5_d_model=384, t5_num_heads=6, t5_d_ff=1024,
                                         t5_num_layers=4).to(dev)
    state = copy.deepcopy(model.state_dict())
    times = {a: [] for a in ARMS}
    peak = {a: 0 for a in ARMS}
    loss = {}
    for _ in range(args.runs):
        for arm in ARMS:
            ms, mem, loss[arm] = block(model, state, batch, arm, args.warmup, args.iters)
            times[arm] += ms
            peak[arm] = max(peak[arm], mem)
    lines = []
    for arm in ARMS:
        lines.append(json.dumps({"attention": arm, "batch": args.batch, "steps_timed": len(times[arm]),
                                 "ms_per_step_median": round(statistics.median(times[arm]), 3),
                                 "ms_per_step_min": round(min(times[arm]), 3),
                                 "peak_allocated_MiB": round(peak[arm] / 2 ** 20, 1),
                                 "last_loss": round(loss[arm], 4)}))
    lines.append(json.dumps({"summary": "torch / hip_train",
                             "median_ratio": round(statistics.median(times["torch"]) /
                                                   statistics.median(times["hip_train"]), 3),
                             "peak_ratio": round(peak["torch"] / peak["hip_train"], 3),
                             "device": torch.cuda.get_device_name(0), "runs": args.runs, "warmup": args.warmup,
                             "iters": args.iters}))
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
