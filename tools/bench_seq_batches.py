#!/usr/bin/env python3
"""Time the retrieval model's input path: what it costs to have one tokenized training batch of the Amazon shape on the
device (batch 640, 20-item windows, 4 ids per item, a 12 101-item corpus, synthetic users), in three arms:

  loader     data.seq_loader.TokenizedSeqLoader: per batch one torch.randint and one ops.seq_batch launch on histories
             that live on the device
  torch_ops  the same windows (same law, same kind of draws) built with torch operators on the device from the same
             resident histories, then the existing SemanticIdTokenizer.forward -- whose range test reads the host
  dataloader torch.utils.data.DataLoader(SeqData, batch_size, shuffle=True) over SeqData.__getitem__ on the host with a
             768-d item matrix, data.utils.batch_to, SemanticIdTokenizer.forward: the reference's shape of input path.
             (Its padded ids are clamped to row 0 before the lookup, one more launch: -1 is no row of the table.)

The arms alternate --runs times in one process on one device; each block is --warmup untimed batches, then --iters
batches with a device event pair around each (the pair encloses the fetch of the batch, so host time during which the
device idles is inside it).  Reports per arm the median batch over all blocks, the median of each block -- their spread
is what a difference between two arms has to exceed -- and the host wall time per batch of each block.  One JSON line
per arm plus a summary line; --out also writes them to a text file.  No threshold is attached to any number.

    python tools/bench_seq_batches.py [--runs 5] [--warmup 3] [--iters 20] [--batch 640] [--arms A,B] [--eval] [--out FILE]

--eval builds evaluation batches (no subsampling, no draw) instead of training batches.

Launches per batch come from kernel traces made in runs of their own, two per arm, each in a fresh process and with no
other tracing:
    rocprofv3 --kernel-trace --output-format csv -d D<K> -o t -- \\
        python tools/bench_seq_batches.py --arms ARM --runs 1 --warmup 1 --iters K          (K = 2 and K = 6)
    python tools/bench_seq_batches.py --count D2 D6
prints (rows of the K = 6 trace - rows of the K = 2 trace) / 4 and the same per kernel name.
"""
import argparse
import csv
import glob
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rq-vae-recommender_amd")]

ARMS = ("loader", "torch_ops", "dataloader")
N_ITEMS, WIDTH, CODES = 12101, 4, 256


def count(dir2, dir6):
    rows = {}
    for k, d in ((2, dir2), (6, dir6)):
        names = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as fh:
                for rec in csv.DictReader(fh):
                    # the name up to its template and argument lists; what tells two such kernels apart (torch's functors)
                    # is kept as a short digest of the whole name
                    full = rec.get("Kernel_Name", "?")
                    name = full.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].split("<")[0].strip() or full[:40]
                    if name != full:
                        name += "#" + hashlib.sha1(full.encode()).hexdigest()[:6]
                    names[name] = names.get(name, 0) + 1
        rows[k] = names
    per = {n: (rows[6].get(n, 0) - rows[2].get(n, 0)) / 4 for n in sorted(set(rows[2]) | set(rows[6]))}
    print(json.dumps({"launches_per_batch": sum(per.values()), "trace_rows_K2": sum(rows[2].values()),
                      "trace_rows_K6": sum(rows[6].values()), "per_kernel": {n: v for n, v in per.items() if v}}))


def torch_ops_batch(seq, rows, draws, S, tokenizer):
    """The window law of data.processed.seq_window in torch operators -> SeqBatch -> the existing tokenizer.forward."""
    import torch
    from data.schemas import SeqBatch
    lo = seq.offsets[rows]
    n_hist = seq.offsets[rows + 1] - lo
    if draws is None:
        count_ = n_hist.clamp_max(S)
        first, fut_pos = n_hist - count_, n_hist
    else:
        n = n_hist + 1
        first = draws[:, 0] % ((n - 3).clamp_min(0) + 1)
        end = torch.minimum(first + 3 + draws[:, 1] % (S - 1), n)
        count_, fut_pos = end - first - 1, end - 1
    pos = torch.arange(S, device=rows.device).unsqueeze(0)
    mask = pos < count_.unsqueeze(1)
    last = seq.items.shape[0] - 1
    ids = seq.items[(lo.unsqueeze(1) + first.unsqueeze(1) + pos).clamp_max(last)].masked_fill(~mask, 0)
    fut = torch.where(fut_pos < n_hist, seq.items[(lo + fut_pos).clamp_max(last)], seq.itemId_fut[rows])
    return tokenizer(SeqBatch(user_ids=seq.userId[rows].unsqueeze(1), ids=ids, ids_fut=fut.unsqueeze(1), x=None, x_fut=None,
                              seq_mask=mask))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=640)
    ap.add_argument("--arms", default=",".join(ARMS), help="comma-separated subset of: " + ", ".join(ARMS))
    ap.add_argument("--eval", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--count", nargs=2, metavar=("DIR_K2", "DIR_K6"), default=None)
    args = ap.parse_args()
    if args.count:
        return count(*args.count)
    arms = args.arms.split(",")
    if not arms or any(a not in ARMS for a in arms):
        ap.error(f"--arms takes names from {list(ARMS)}")

    import torch
    from torch.utils.data import DataLoader

    from data.processed import RecDataset, SeqData, synthetic_item_matrix
    from data.seq_loader import TokenizedSeqLoader
    from data.utils import batch_to, cycle
    from modules.tokenizer.semids import SemanticIdTokenizer

    dev = torch.device("cuda")
    folder, train = f"synthetic:{N_ITEMS}", not args.eval
    tok = SemanticIdTokenizer(input_dim=16, output_dim=8, hidden_dims=[16], codebook_size=CODES, n_layers=WIDTH - 1, n_cat_feats=0)
    tok.cached_ids = torch.randint(0, CODES, (N_ITEMS, WIDTH), generator=torch.Generator().manual_seed(1)).to(dev)
    resident = SeqData(folder, dataset=RecDataset.AMAZON, is_train=train, subsample=train).to_device(dev)
    S, B, U = resident.max_seq_len, args.batch, len(resident)

    def loader_arm():
        return cycle(TokenizedSeqLoader(resident, tok, B, shuffle=True))

    def torch_ops_arm():
        while True:
            perm = torch.randperm(U, device=dev)
            for start in range(0, U, B):
                rows = perm[start:start + B]
                draws = torch.randint(0, 2 ** 62, (rows.shape[0], 2), dtype=torch.int64, device=dev) if train else None
                yield torch_ops_batch(resident, rows, draws, S, tok)

    def dataloader_arm():
        host = SeqData(folder, dataset=RecDataset.AMAZON, is_train=train, subsample=train,
                       item_matrix=synthetic_item_matrix(N_ITEMS))
        for raw in cycle(DataLoader(host, batch_size=B, shuffle=True)):
            batch = batch_to(raw, dev)
            yield tok(batch._replace(ids=batch.ids.clamp_min(0)))

    make = {"loader": loader_arm, "torch_ops": torch_ops_arm, "dataloader": dataloader_arm}
    streams = {a: make[a]() for a in arms}
    times = {a: [] for a in arms}
    blocks = {a: [] for a in arms}
    wall = {a: [] for a in arms}
    for _ in range(args.runs):
        for arm in arms:
            ms = []
            for it in range(args.warmup + args.iters):
                if it == args.warmup:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                batch = next(streams[arm])
                stop.record()
                stop.synchronize()
                if it >= args.warmup:
                    ms.append(start.elapsed_time(stop))
            wall[arm].append(round((time.perf_counter() - t0) * 1e3 / args.iters, 3))
            assert batch.sem_ids.shape[1] == S * WIDTH and batch.sem_ids_fut.shape[1] == WIDTH
            times[arm] += ms
            blocks[arm].append(round(statistics.median(ms), 4))
    lines = []
    for arm in arms:
        lines.append(json.dumps({"arm": arm, "batches": "train" if train else "eval", "batch": B, "S": S, "w": WIDTH,
                                 "items": N_ITEMS, "users": U, "batches_timed": len(times[arm]),
                                 "ms_per_batch_median": round(statistics.median(times[arm]), 4),
                                 "ms_per_batch_min": round(min(times[arm]), 4), "block_medians": blocks[arm],
                                 "host_wall_ms_per_batch_by_block": wall[arm]}))
    summary = {"summary": "median batch, arm / loader", "device": torch.cuda.get_device_name(0), "runs": args.runs,
               "warmup": args.warmup, "iters": args.iters}
    if "loader" in arms:
        for a in arms:
            if a != "loader":
                summary[f"{a} / loader"] = round(statistics.median(times[a]) / statistics.median(times["loader"]), 2)
    lines.append(json.dumps(summary))
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
