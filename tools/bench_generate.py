#!/usr/bin/env python3
"""Time EncoderDecoderRetrievalModel.generate at the Amazon decoder config (d_model 384, 6 heads, d_ff 1024, 4 layers,
K = 256, L = 3, k = 10, batch 640, 20-item histories, a 12 101-item corpus), two ways:

  kernel     the model as built: each hierarchy step is the decoder, the head and one ops.beam_step launch
  reference  the same model with the beam step replaced by the reference's operator sequence (softmax,
             torch.multinomial, gather, log, the [N, P, h] prefix-equality test in chunks of 100 000, masked_fill,
             sort, gathers and a cat)

and, for the kernel path, with either attention implementation (--attention): "torch", the T5 operators, or "hip",
one ops.t5_attention launch per attention call and slab K/V (modules/t5.py).  `--attention both` alternates the two
arms --runs times in one process and ends with one summary line of the medians over the runs.  --proj sets proj_impl
(modules/t5.py) for every arm: "hip" makes the attention projections grouped ops.t5_proj_fwd launches, the decode
step's K/V written by them straight into the cache slabs; --ffn sets ffn_impl likewise.  --arith sets matmul_arith, the
arithmetic of those two "hip" forms ("bf16": bf16 operands, fp32 accumulation); `--arith both` alternates fp32 and bf16
--runs times on one --attention arm of the kernel path and ends with a summary line.  --beam sets beam_impl
(modules/model.py) of the kernel path: "sample", the reference's sampling search (a noise draw and one ops.beam_step per
level), or "exact", the deterministic constrained search (one ops.beam_topk_step per level, no noise); `--beam both`
alternates the two --runs times on one --attention arm and ends with a summary line of the medians over the runs' block
medians and their spread.  --images sets weight_images (modules/t5.py) under `--arith bf16` on the kernel path: "bf16" reads
the weights of the two "hip" forms from bf16 images; `--images both` alternates "none" and "bf16" --runs times and ends
with a summary line of the medians over the runs' block medians and their spread.
--rows sets encoder_rows (modules/model.py) of the kernel path under --attention hip: "packed" runs the encoder, the cross
K/V and every decode step's cross-attention on the valid tokens only.  It times --batches counted batches of --batch users
from data.seq_loader.TokenizedSeqLoader(host_windows=True) over the synthetic:12101 histories, cycled: --fill eval = the
eval split's whole histories (fill about 0.75), --fill train = histories cut by the training window law (about 0.35).
`--rows padded,packed` alternates the two arms --runs times in one process (the rule of
profiles/retrieval_train_step_proj.txt) and ends with a summary line: per arm the median over the block medians, their
spread and the peak allocated memory.  --norm and --embed set norm_impl and embed_impl there.

Device events around each generate after a warm-up; prints one JSON line per path (ms per generate, users/s).
Kernel launches per generate come from a separate `rocprofv3 --kernel-trace --stats` run of this tool
(--path one of them, one --attention arm, --iters small).

    python tools/bench_generate.py [--path kernel|reference|both] [--attention torch|hip|both] [--runs 5]
                                   [--proj torch|hip] [--ffn torch|hip] [--arith fp32|bf16|both]
                                   [--images none|bf16|both] [--beam sample|exact|both] [--warmup 3] [--iters 10]
                                   [--rows padded|packed|padded,packed] [--fill eval|train] [--batch 640] [--batches 4]
                                   [--norm torch|hip] [--embed torch|hip]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rq-vae-recommender_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import modules.model as mm  # noqa: E402
from retrieval_cases import synthetic_batch, to_device  # noqa: E402  (tests/retrieval_cases.py)


def reference_beam_step(corpus):
    """The reference's per-step operators (modules/model.py generate), in the signature of ops.beam_step."""

    def check_valid_prefix(prefix, batch_size=100000):
        trimmed = corpus[:, : prefix.shape[1]]
        out = []
        for i in range(0, prefix.shape[0], batch_size):
            chunk = prefix[i: i + batch_size]
            out.append((trimmed.unsqueeze(1) == chunk.unsqueeze(0)).all(dim=2).any(dim=0))
        return torch.cat(out)

    def step(logits, noise, parent_scores, parent_ids, index, corpus_, n_cands, k):
        probas = F.softmax(logits, dim=-1)
        samples = torch.multinomial(probas, num_samples=n_cands)
        samp_log_p = torch.log(torch.gather(probas, 1, samples))
        if parent_ids is None:
            B = logits.shape[0]
            is_valid = check_valid_prefix(samples.reshape(-1, 1)).reshape(B, n_cands)
            scores, idx = samp_log_p.masked_fill(~is_valid, float("-inf")).sort(-1, descending=True)
            top = idx[:, :k]
            ids = torch.gather(samples, 1, top).unsqueeze(-1)
            parent = torch.arange(B, device=logits.device).unsqueeze(1).expand(-1, k)
            return ids, scores[:, :k], parent
        B, beams, h = parent_ids.shape
        prev = parent_ids.reshape(-1, h).repeat_interleave(n_cands, dim=0)
        prefix = torch.cat([prev, samples.reshape(-1, 1)], dim=1)
        is_valid = check_valid_prefix(prefix).reshape(B, beams * n_cands)
        scores, idx = ((samp_log_p.reshape(B, beams * n_cands) + parent_scores.repeat_interleave(n_cands, dim=1))
                       .masked_fill(~is_valid, float("-inf")).sort(-1, descending=True))
        top = idx[:, :k]
        parent_beam = top // n_cands
        parent = parent_beam + torch.arange(B, device=logits.device).unsqueeze(1) * beams
        pids = torch.gather(parent_ids, 1, parent_beam.unsqueeze(-1).expand(-1, -1, h))
        new = torch.gather(samples.reshape(B, beams * n_cands), 1, top).unsqueeze(-1)
        return torch.cat([pids, new], dim=-1), scores[:, :k], parent

    return step


def build(dev, B=640, items=20, N=12101, L=3, K=256, seed=0):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    corpus = torch.randint(0, K, (N, L), generator=g)
    model = mm.EncoderDecoderRetrievalModel(corpus, L, K, t5_d_model=384, t5_num_heads=6, t5_d_ff=1024,
                                            t5_num_layers=4, top_k_for_generation=10).to(dev).eval()
    return model, to_device(synthetic_batch(corpus, B, items, g, user_ids=False), dev)


def time_path(model, batch, warmup, iters):
    for _ in range(warmup):
        model.generate_next_sem_id(batch)
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        model.generate_next_sem_id(batch)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], times[0]


def loader_batches(corpus, B, n, dev, law, seed=0):
    """n counted batches of B rows from TokenizedSeqLoader(host_windows=True) over the synthetic histories of the corpus'
    size: law "eval" = the eval split as evaluate_decoder.py reads it (whole histories up to the 20 slots), "train" = the
    same histories cut by the training window law (subsample).  -> (batches, fill: valid items / item slots)."""
    from data.processed import RecDataset, SeqData
    from data.seq_loader import TokenizedSeqLoader
    from modules.tokenizer.semids import SemanticIdTokenizer
    N, L = corpus.shape
    train = law == "train"
    ds = SeqData(root=f"synthetic:{N}", dataset=RecDataset.AMAZON, is_train=train, subsample=train).to_device(dev)
    tok = SemanticIdTokenizer(input_dim=16, output_dim=8, hidden_dims=[16], codebook_size=256, n_layers=L, n_cat_feats=0)
    tok.cached_ids = torch.cat([corpus, torch.zeros(N, 1, dtype=torch.long)], dim=1).to(dev)
    torch.manual_seed(seed)
    out = []
    for batch in TokenizedSeqLoader(ds, tok, B, shuffle=True, host_windows=True):
        if batch.sem_ids.shape[0] == B:
            out.append(batch)
        if len(out) == n:
            break
    fill = sum(float(b.item_counts.sum()) for b in out) / (len(out) * B * ds.max_seq_len)
    return out, fill


def rows_block(model, batches, rows, warmup, iters):
    """One block of one --rows arm -> (ms per generate of the timed calls, peak allocated bytes)."""
    model.encoder_rows = rows
    for i in range(warmup):
        model.generate_next_sem_id(batches[i % len(batches)])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for i in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        model.generate_next_sem_id(batches[i % len(batches)])
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return times, torch.cuda.max_memory_allocated()


def compare_rows(args, model, dev):
    """--rows: the arms (encoder_rows of modules/model.py) alternate --runs times in this process over the same counted
    batches; one line per block, then one summary line: per arm the median of the block medians, their spread
    (max - min) and the peak memory."""
    arms = args.rows.split(",")
    batches, fill = loader_batches(model.codebooks.cpu(), args.batch, args.batches, dev, args.fill)
    model.attention_impl, model.matmul_arith, model.beam_impl = args.attention, args.arith, args.beam
    if "packed" in arms:      # a batch that fell back to the padded path, silently, would be timed as packed
        model.encoder_rows = "packed"
        L = model.num_hierarchies
        with torch.no_grad():      # as `generate` asks
            plans = [model.packed_rows_plan(b.item_counts, b.sem_ids, b.user_ids is not None, ld_item=L + 1,
                                            query_length=1) for b in batches]
        if any(plan is None for plan in plans):
            raise SystemExit("--rows packed: a batch of this run would take the padded path (modules/model.py)")
    common = {"path": "kernel", "attention": args.attention, "proj": args.proj, "ffn": args.ffn, "norm": args.norm,
              "embed": args.embed, "arith": args.arith, "beam": args.beam, "batch": args.batch, "fill_law": args.fill,
              "fill": round(fill, 4), "batches": len(batches)}
    medians, peaks = {arm: [] for arm in arms}, {arm: 0 for arm in arms}
    for run in range(args.runs):
        for arm in arms:
            times, peak = rows_block(model, batches, arm, args.warmup, args.iters)
            times.sort()
            medians[arm].append(times[len(times) // 2])
            peaks[arm] = max(peaks[arm], peak)
            print(json.dumps({**common, "rows": arm, "run": run, "ms_per_generate_median": round(medians[arm][-1], 3),
                              "ms_per_generate_min": round(times[0], 3), "peak_allocated_MiB": round(peak / 2 ** 20, 1),
                              "iters": args.iters}), flush=True)
    mid = {arm: sorted(v)[len(v) // 2] for arm, v in medians.items()}
    print(json.dumps({**common, "rows": args.rows, "runs": args.runs,
                      **{f"block_medians_{arm}": [round(v, 3) for v in medians[arm]] for arm in arms},
                      **{f"ms_per_generate_{arm}": round(mid[arm], 3) for arm in arms},
                      **{f"spread_{arm}": round(max(medians[arm]) - min(medians[arm]), 3) for arm in arms},
                      **{f"peak_allocated_MiB_{arm}": round(peaks[arm] / 2 ** 20, 1) for arm in arms},
                      **({"padded_over_packed": round(mid["padded"] / mid["packed"], 4)} if len(arms) == 2 else {}),
                      "device": torch.cuda.get_device_name(0)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", choices=["padded", "packed", "padded,packed"], default=None,
                    help="encoder_rows of the kernel path on counted loader batches (--fill); padded,packed alternates the "
                         "two --runs times and ends with a summary line")
    ap.add_argument("--fill", choices=["eval", "train"], default="eval",
                    help="with --rows: whole eval histories (fill about 0.75) or histories cut by the training window law "
                         "(about 0.35)")
    ap.add_argument("--batch", type=int, default=640, help="with --rows: users per generate")
    ap.add_argument("--batches", type=int, default=4, help="with --rows: loader batches, drawn once and cycled")
    ap.add_argument("--norm", choices=["torch", "hip"], default="torch", help="with --rows: norm_impl")
    ap.add_argument("--embed", choices=["torch", "hip"], default="torch", help="with --rows: embed_impl")
    ap.add_argument("--path", choices=["kernel", "reference", "both"], default=None,
                    help="default: both, or kernel with --attention both")
    ap.add_argument("--attention", choices=["torch", "hip", "both"], default="torch")
    ap.add_argument("--proj", choices=["torch", "hip"], default="torch", help="proj_impl of every arm")
    ap.add_argument("--ffn", choices=["torch", "hip"], default="torch", help="ffn_impl of every arm")
    ap.add_argument("--arith", choices=["fp32", "bf16", "both"], default="fp32",
                    help='matmul_arith of the "hip" projections and feed-forward')
    ap.add_argument("--images", choices=["none", "bf16", "both"], default="none",
                    help='weight_images of the "hip" projections and feed-forward under --arith bf16; both alternates')
    ap.add_argument("--beam", choices=["sample", "exact", "both"], default="sample", help="beam_impl of the kernel path")
    ap.add_argument("--runs", type=int, default=5,
                    help="alternations of the two arms with --attention / --arith / --beam both")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    if args.rows is not None:
        if args.attention != "hip" or args.arith == "both" or args.beam == "both" or args.images != "none" or \
                args.path not in (None, "kernel"):
            ap.error("--rows applies to --path kernel with --attention hip, one --arith and one --beam")
        dev = torch.device("cuda")
        model, _ = build(dev, B=1)
        model.proj_impl, model.ffn_impl, model.norm_impl, model.embed_impl = args.proj, args.ffn, args.norm, args.embed
        compare_rows(args, model, dev)
        return
    if args.path is None:
        args.path = "kernel" if args.attention == "both" or args.beam != "sample" else "both"
    dev = torch.device("cuda")
    model, batch = build(dev)
    model.proj_impl, model.ffn_impl = args.proj, args.ffn
    B = batch.sem_ids.shape[0]
    paths = ["kernel", "reference"] if args.path == "both" else [args.path]
    if args.beam != "sample" and (args.path != "kernel" or args.arith == "both" or args.attention == "both"):
        ap.error("--beam exact / both applies to --path kernel on one --attention arm and one --arith")
    if args.beam == "both":
        model.attention_impl, model.matmul_arith = args.attention, args.arith
        medians = {"sample": [], "exact": []}
        for run in range(args.runs):
            for arm in ("sample", "exact"):
                model.beam_impl = arm
                med, best = time_path(model, batch, args.warmup, args.iters)
                medians[arm].append(med)
                print(json.dumps({"path": "kernel", "attention": args.attention, "proj": args.proj, "ffn": args.ffn,
                                  "arith": args.arith, "beam": arm, "run": run, "batch": B,
                                  "ms_per_generate_median": round(med, 3), "ms_per_generate_min": round(best, 3),
                                  "iters": args.iters}), flush=True)
        mid = {arm: sorted(v)[len(v) // 2] for arm, v in medians.items()}
        print(json.dumps({"path": "kernel", "attention": args.attention, "proj": args.proj, "ffn": args.ffn,
                          "arith": args.arith, "beam": "both", "runs": args.runs, "batch": B,
                          "run_medians_sample": [round(v, 3) for v in medians["sample"]],
                          "run_medians_exact": [round(v, 3) for v in medians["exact"]],
                          "ms_per_generate_sample": round(mid["sample"], 3), "ms_per_generate_exact": round(mid["exact"], 3),
                          "spread_sample": round(max(medians["sample"]) - min(medians["sample"]), 3),
                          "spread_exact": round(max(medians["exact"]) - min(medians["exact"]), 3),
                          "exact_over_sample": round(mid["exact"] / mid["sample"], 4)}), flush=True)
        return
    model.beam_impl = args.beam
    if args.images != "none":
        if args.arith != "bf16" or args.attention == "both" or args.path != "kernel":
            ap.error("--images bf16 / both applies to --path kernel with --arith bf16 on one --attention arm")
        model.attention_impl, model.matmul_arith = args.attention, "bf16"
        arms = ("none", "bf16") if args.images == "both" else ("bf16",)
        medians = {arm: [] for arm in arms}
        for run in range(args.runs):
            for arm in arms:
                model.weight_images = arm
                med, best = time_path(model, batch, args.warmup, args.iters)
                medians[arm].append(med)
                print(json.dumps({"path": "kernel", "attention": args.attention, "proj": args.proj, "ffn": args.ffn,
                                  "arith": "bf16", "images": arm, "beam": args.beam, "run": run, "batch": B,
                                  "ms_per_generate_median": round(med, 3), "ms_per_generate_min": round(best, 3),
                                  "iters": args.iters}), flush=True)
        mid = {arm: sorted(v)[len(v) // 2] for arm, v in medians.items()}
        print(json.dumps({"path": "kernel", "attention": args.attention, "proj": args.proj, "ffn": args.ffn,
                          "arith": "bf16", "images": args.images, "beam": args.beam, "runs": args.runs, "batch": B,
                          **{f"run_medians_{arm}": [round(v, 3) for v in medians[arm]] for arm in arms},
                          **{f"ms_per_generate_{arm}": round(mid[arm], 3) for arm in arms},
                          **{f"spread_{arm}": round(max(medians[arm]) - min(medians[arm]), 3) for arm in arms},
                          **({"bf16_over_none": round(mid["bf16"] / mid["none"], 4)} if len(arms) == 2 else {})}),
              flush=True)
        return
    if args.arith == "both":
        if args.attention == "both" or args.path not in ("kernel", "both"):
            ap.error("--arith both compares the two arithmetics on one --attention arm of --path kernel")
        model.attention_impl = args.attention
        medians = {"fp32": [], "bf16": []}
        for run in range(args.runs):
            for arm in ("fp32", "bf16"):
                model.matmul_arith = arm
                med, best = time_path(model, batch, args.warmup, args.iters)
                medians[arm].append(med)
                print(json.dumps({"path": "kernel", "attention": args.attention, "proj": args.proj, "ffn": args.ffn,
                                  "arith": arm, "run": run, "batch": B, "ms_per_generate_median": round(med, 3),
                                  "ms_per_generate_min": round(best, 3), "iters": args.iters}), flush=True)
        mid = {arm: sorted(v)[len(v) // 2] for arm, v in medians.items()}
        print(json.dumps({"path": "kernel", "attention": args.attention, "proj": args.proj, "ffn": args.ffn,
                          "arith": "both", "runs": args.runs, "batch": B, "run_medians_fp32": [round(v, 3) for v in medians["fp32"]],
                          "run_medians_bf16": [round(v, 3) for v in medians["bf16"]],
                          "ms_per_generate_fp32": round(mid["fp32"], 3), "ms_per_generate_bf16": round(mid["bf16"], 3),
                          "bf16_over_fp32": round(mid["bf16"] / mid["fp32"], 4)}), flush=True)
        return
    model.matmul_arith = args.arith
    if args.attention == "both":
        if args.path != "kernel":
            ap.error("--attention both compares the two arms of --path kernel")
        medians = {"torch": [], "hip": []}
        for run in range(args.runs):
            for arm in ("torch", "hip"):
                model.attention_impl = arm
                med, best = time_path(model, batch, args.warmup, args.iters)
                medians[arm].append(med)
                print(json.dumps({"path": "kernel", "attention": arm, "proj": args.proj, "ffn": args.ffn,
                                  "arith": args.arith, "run": run, "batch": B,
                                  "ms_per_generate_median": round(med, 3), "ms_per_generate_min": round(best, 3),
                                  "iters": args.iters}), flush=True)
        mid = {arm: sorted(v)[len(v) // 2] for arm, v in medians.items()}
        print(json.dumps({"path": "kernel", "attention": "both", "runs": args.runs, "batch": B,
                          "ms_per_generate_torch": round(mid["torch"], 3), "ms_per_generate_hip": round(mid["hip"], 3),
                          "hip_over_torch": round(mid["hip"] / mid["torch"], 4)}), flush=True)
        return
    model.attention_impl = args.attention
    for path in paths:
        if path == "reference":
            mm.ops.beam_step, saved = reference_beam_step(model.codebooks), mm.ops.beam_step
            mm._exponential_like, saved_q = (lambda p: p), mm._exponential_like  # multinomial draws its own noise
        try:
            med, best = time_path(model, batch, args.warmup, args.iters)
        finally:
            if path == "reference":
                mm.ops.beam_step, mm._exponential_like = saved, saved_q
        print(json.dumps({"path": path, "attention": args.attention, "proj": args.proj, "ffn": args.ffn,
                          "arith": args.arith, "beam": model.beam_impl if path == "kernel" else "sample", "batch": B,
                          "k": model.top_k_for_generation, "L": model.num_hierarchies,
                          "K": model.num_embeddings_per_hierarchy, "corpus": int(model.codebooks.shape[0]),
                          "ms_per_generate_median": round(med, 3), "ms_per_generate_min": round(best, 3),
                          "users_per_s": round(B / (med / 1e3), 1), "iters": args.iters}), flush=True)


if __name__ == "__main__":
    main()
