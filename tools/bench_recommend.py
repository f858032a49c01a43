#!/usr/bin/env python3
"""The expansion of generated semantic-id tuples to corpus items (csrc/sid_items.hip, SemIdItemIndex.expand) on one
MI355X, two arms alternating in one process:

  kernel     ops.sid_items_topn: ONE launch per call
  operators  the same expansion written with torch operators on the device (`OperatorExpander` below, which lives in this
             tool only): key packing, searchsorted, a ragged expansion on a fixed [B, k, n + T] grid, the history mask
             and a per-user compaction by cumsum and scatter -- static shapes, nothing read by the host

Shapes: batch 640, a synthetic 12 101-row corpus over 256^3 codes with planted collision groups (400 groups of 2 to 31
items), histories of 20 items of which half come from the user's own beams' groups; k = n = 10, and k = 64, n = 50.
Both arms are checked for torch.equal outputs before anything is timed.

    python tools/bench_recommend.py                    time per call: --runs alternations of both arms, each run the median
                                                       of --blocks blocks of --calls calls between two device events
    rocprofv3 --kernel-trace --output-format csv -d D -o t -- python tools/bench_recommend.py --trace
                                                       a run of its own for the profiler: --calls calls of each arm and
                                                       shape and ONE generate at batch 640 (the Amazon decoder config,
                                                       beam_impl "exact", attention_impl "hip"), the phases separated by
                                                       a marker launch (fill_u8_kernel)
    python tools/bench_recommend.py --summarize D/**/t_kernel_trace.csv --calls N
                                                       launches per call of each arm and the kernel's share of one
                                                       generate's kernel time, from that trace
    python tools/bench_recommend.py --metrics          a short train_decoder.train on `synthetic:2000`, then
                                                       recommend.recommend: how far item-level and tuple-level h@k differ
"""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rq-vae-recommender_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402

N_ITEMS, K_CODES, L, BATCH, T_HIST = 12101, 256, 3, 640, 20
SHAPES = ((10, 10), (64, 50))      # (k, n)
MARKER = "fill_u8_kernel"


def synthetic_corpus(g):
    """[N, L] host tensor: uniform codes, then 400 planted groups of 2 .. 31 rows that share one tuple."""
    corpus = torch.randint(0, K_CODES, (N_ITEMS, L), generator=g)
    for group in range(400):
        rows = torch.randint(0, N_ITEMS, (2 + group % 30,), generator=g)
        corpus[rows] = corpus[rows[0]].clone()
    return corpus


def host_ranks(corpus):
    seen, out = {}, []
    for row in corpus.tolist():
        key = tuple(row)
        out.append(seen.get(key, 0))
        seen[key] = out[-1] + 1
    return torch.tensor(out)


def inputs(corpus, ranks, k, g):
    """beams [B, k, L], scores [B, k] descending with a few -inf at the end, history [B, T * (L + 1)] with real ranks."""
    picked = torch.randint(0, N_ITEMS, (BATCH, k), generator=g)
    beams = corpus[picked]
    scores = -torch.rand(BATCH, k, generator=g).cumsum(dim=1)
    if k >= 8:
        scores[:, k - k // 8:] = float("-inf")
    seen = torch.randint(0, N_ITEMS, (BATCH, T_HIST), generator=g)
    seen[:, : T_HIST // 2] = picked[:, torch.arange(T_HIST // 2) % k]       # items of the user's own beams' groups
    cached = torch.cat([corpus, ranks[:, None]], dim=1)
    history = cached[seen]
    history[torch.rand(BATCH, T_HIST, generator=g) < 0.1] = -1              # padding
    return beams, scores, history.reshape(BATCH, -1)


class OperatorExpander:
    """rqhip_sid_items_topn's semantics (include/rqhip.h) with torch operators, for codes < K_CODES."""

    def __init__(self, corpus):
        self.N = corpus.shape[0]
        self.weights = K_CODES ** torch.arange(L - 1, -1, -1, device=corpus.device)
        # a stable sort by tuple: inside a group ascending item number == ascending dedup rank
        self.keys, self.order = torch.sort((corpus * self.weights).sum(-1), stable=True)

    def expand(self, beams, scores, n, history=None):
        B, k, _ = beams.shape
        dev = beams.device
        key = (beams * self.weights).sum(-1)
        lo = torch.searchsorted(self.keys, key)
        hi = torch.searchsorted(self.keys, key, right=True)
        live = scores > float("-inf")
        earlier = torch.ones(k, k, dtype=torch.bool, device=dev).tril(-1)
        live = live & ~((key[:, :, None] == key[:, None, :]) & live[:, None, :] & earlier).any(-1)
        T = 0 if history is None else history.shape[1] // (L + 1)
        cap = n + T                                     # at most T ranks of a group are skipped before n are found
        count = torch.where(live, hi - lo, torch.zeros_like(lo)).clamp(max=cap)
        r = torch.arange(cap, device=dev)
        valid = r < count[..., None]
        item = self.order[(lo[..., None] + r).clamp(max=self.N - 1)]
        if T:
            h = history.view(B, T, L + 1)
            hkey, hrank = (h[..., :L] * self.weights).sum(-1), h[..., L]
            at = torch.searchsorted(self.keys, hkey) + hrank.clamp(min=0)
            pos = at.clamp(max=self.N - 1)
            real = (h >= 0).all(-1) & (at < self.N) & (self.keys[pos] == hkey)
            seen = torch.where(real, self.order[pos], torch.full_like(pos, -2))
            valid = valid & ~(item[..., None] == seen[:, None, None, :]).any(-1)
        valid, item = valid.reshape(B, -1), item.reshape(B, -1)
        score = scores[:, :, None].expand(B, k, cap).reshape(B, -1)
        slot = valid.cumsum(1) - 1
        keep = valid & (slot < n)
        slot = torch.where(keep, slot, torch.full_like(slot, n))            # column n collects what is dropped
        items = torch.full((B, n + 1), -1, dtype=torch.int64, device=dev).scatter_(
            1, slot, torch.where(keep, item, torch.full_like(item, -1)))
        item_scores = torch.full((B, n + 1), float("-inf"), device=dev).scatter_(
            1, slot, torch.where(keep, score, torch.full_like(score, float("-inf"))))
        return items[:, :n].contiguous(), item_scores[:, :n].contiguous()


def setup(dev):
    from modules.sid_items import SemIdItemIndex
    g = torch.Generator().manual_seed(0)
    corpus = synthetic_corpus(g)
    ranks = host_ranks(corpus)
    index = SemIdItemIndex(corpus.to(dev))
    assert torch.equal(index.ranks.cpu(), ranks)
    operators = OperatorExpander(corpus.to(dev))
    cases = {}
    for k, n in SHAPES:
        beams, scores, history = (t.to(dev) for t in inputs(corpus, ranks, k, g))
        got, want = index.expand(beams, scores, n, history), operators.expand(beams, scores, n, history)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (k, n)
        cases[(k, n)] = (beams, scores, history)
    groups = torch.unique(corpus, dim=0, return_counts=True)[1]
    print(f"corpus: {N_ITEMS} rows over {K_CODES}^{L} codes, {int((groups > 1).sum())} tuples shared by "
          f"{int(groups[groups > 1].sum())} rows (largest group {int(groups.max())}); batch {BATCH}, history {T_HIST} items; "
          f"index {index._index.numel() / 1024:.0f} KiB; both arms give torch.equal outputs", flush=True)
    return index, operators, cases


def per_call_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def time_arms(args):
    index, operators, cases = setup(torch.device("cuda"))
    for (k, n), case in cases.items():
        arms = {"kernel": lambda: index.expand(case[0], case[1], n, case[2]),
                "operators": lambda: operators.expand(case[0], case[1], n, case[2])}
        for fn in arms.values():
            per_call_ms(fn, 10)
        medians = {arm: [] for arm in arms}
        for run in range(args.runs):
            for arm, fn in arms.items():
                medians[arm].append(statistics.median(per_call_ms(fn, args.calls) for _ in range(args.blocks)))
        out = {"k": k, "n": n, "batch": BATCH, "runs": args.runs, "blocks": args.blocks, "calls_per_block": args.calls}
        for arm, v in medians.items():
            out[f"us_per_call_{arm}"] = round(statistics.median(v) * 1e3, 2)
            out[f"run_medians_us_{arm}"] = [round(x * 1e3, 2) for x in v]
            out[f"spread_us_{arm}"] = round((max(v) - min(v)) * 1e3, 2)
        out["operators_over_kernel"] = round(statistics.median(medians["operators"]) / statistics.median(medians["kernel"]), 1)
        print(json.dumps(out), flush=True)


def make_marker(dev):
    """-> a function that makes one launch of a kernel nothing else here uses (rqhip_prefix_lookup at h = 0 is a fill) and
    no other launch: its tensors are made here."""
    from rqhip import ops
    corpus = torch.zeros(64, 1, dtype=torch.int64, device=dev)
    index = ops.prefix_index_build(corpus)
    empty = torch.zeros(8, 0, dtype=torch.int64, device=dev)
    return lambda: ops.prefix_lookup(index, corpus, empty)


def trace(args):
    """For rocprofv3: marker, then per phase its calls and a marker.  Phases: kernel and operators per shape, generate."""
    from bench_generate import build
    dev = torch.device("cuda")
    index, operators, cases = setup(dev)
    model, batch = build(dev)
    model.beam_impl, model.attention_impl = "exact", "hip"
    model.generate_next_sem_id(batch)                                       # warm-up of every phase's shapes
    marker = make_marker(dev)
    torch.cuda.synchronize()
    marker()
    for (k, n), case in cases.items():
        for arm in (index, operators):
            for _ in range(args.calls):
                arm.expand(case[0], case[1], n, case[2])
            marker()
    model.generate_next_sem_id(batch)
    marker()
    torch.cuda.synchronize()
    print(f"trace: {args.calls} calls per phase", flush=True)


def summarize(args):
    rows = []
    with open(args.summarize) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    marks = [i for i, r in enumerate(rows) if MARKER in r[2]]
    names = [f"{arm} k={k} n={n}" for k, n in SHAPES for arm in ("kernel", "operators")] + ["generate"]
    assert len(marks) >= len(names) + 1, f"{len(marks)} marker launches in the trace, {len(names) + 1} expected"
    marks = marks[-(len(names) + 1):]
    kernel_us = {}
    for name, a, b in zip(names, marks[:-1], marks[1:]):
        phase = rows[a + 1:b]
        calls = 1 if name == "generate" else args.calls
        busy = sum(e - s for s, e, _ in phase) / 1e3
        print(f"{name}: {len(phase)} dispatches in {calls} call(s) = {len(phase) / calls:g} per call; kernel time "
              f"{busy / calls:.1f} us per call")
        kernel_us[name] = busy / calls
        if name.startswith("kernel"):
            print("    dispatched: " + ", ".join(sorted({r[2].split("(")[0] for r in phase})))
            assert all("items_topn_kernel" in r[2] for r in phase), name
    gen = kernel_us["generate"]
    for k, n in SHAPES:
        share = kernel_us[f"kernel k={k} n={n}"] / gen
        print(f"items_topn_kernel k={k} n={n}: {100 * share:.3f} % of one generate's kernel time ({gen / 1e3:.2f} ms, "
              f"batch {BATCH}, k = 10)")


def metrics(args):
    import tempfile

    import recommend
    import train_decoder
    from data.processed import RecDataset
    from modules.tokenizer.semids import SemanticIdTokenizer
    with tempfile.TemporaryDirectory() as tmp:
        root = tmp + "/"
        cfg = dict(dataset_folder="synthetic:2000", dataset=RecDataset.AMAZON, batch_size=64, iterations=args.iterations,
                   partial_eval_every=args.iterations, full_eval_every=args.iterations, log_every=args.iterations,
                   learning_rate=0.001, weight_decay=0.0001, max_grad_norm=1.0, vae_input_dim=768, vae_hidden_dims=[32],
                   vae_embed_dim=16, vae_codebook_size=16, vae_n_layers=3, vae_n_cat_feats=0, t5_d_model=64,
                   t5_num_heads=2, t5_d_ff=128, t5_num_layers=2, top_k_for_generation=10, top_k_eval_list=[1, 5, 10],
                   save_dir_root=root)
        torch.manual_seed(0)
        tok = SemanticIdTokenizer(input_dim=768, hidden_dims=[32], output_dim=16, codebook_size=16, n_layers=3, n_cat_feats=0)
        torch.save({"iter": 0, "model": tok.rq_vae.state_dict()}, root + "rqvae.pt")
        cfg["pretrained_rqvae_path"] = root + "rqvae.pt"
        torch.manual_seed(0)
        checkpoint = train_decoder.train(**cfg)["checkpoint"]
        import inspect
        params = inspect.signature(recommend.recommend).parameters
        shared = {name: v for name, v in cfg.items() if name in params}
        for exclude in (False, True):
            res = recommend.recommend(checkpoint_path=checkpoint, n_items=10, exclude_history=exclude, **shared)
            print(json.dumps({"corpus": "synthetic:2000, untrained RQ-VAE with 16^3 codes", "train_iterations": args.iterations,
                              "exclude_history": exclude, **res}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarize", default=None, metavar="KERNEL_TRACE_CSV")
    ap.add_argument("--metrics", action="store_true")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=None, help="calls per block (default 50), or per traced phase (default 5)")
    ap.add_argument("--iterations", type=int, default=200, help="training steps before --metrics")
    args = ap.parse_args()
    if args.calls is None:
        args.calls = 5 if args.trace or args.summarize else 50
    if args.summarize:
        return summarize(args)
    if not torch.cuda.is_available():
        raise SystemExit("bench_recommend needs a ROCm GPU: nothing here is measured on a CPU")
    if args.trace:
        return trace(args)
    if args.metrics:
        return metrics(args)
    return time_arms(args)


if __name__ == "__main__":
    main()
