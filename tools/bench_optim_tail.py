#!/usr/bin/env python3
"""Time the optimizer tail of the retrieval model's training loop by itself -- clip the global gradient norm to 1.0,
AdamW, one step of the inverse-square-root schedule (reference train_decoder.py:147-151, 202-205) -- on the parameter
list of the Amazon decoder config (d_model 384, 6 heads, d_ff 1024, 4 layers, K = 256, L = 3) with fixed random
gradients: no forward, no backward.  The decoder stack's embed_tokens has no gradient, as in training.  Four arms:

  torch_foreach  torch.nn.utils.clip_grad_norm_(params, 1.0) + torch.optim.AdamW(foreach=True).step() + scheduler.step()
  torch_fused    the same with torch.optim.AdamW(fused=True)
  tail_eager     rqhip.optim.FlatAdamW(max_grad_norm=1.0).step() + scheduler.step(): csrc/adamw.hip:rqhip_adamw_tail_step
                 (sum of squares, one scalar kernel, update; norm, clip coefficient and learning rate stay on the device)
  tail_graph     the same optimizer step captured once into a hipGraph; per tail one replay + the host-only scheduler.step()

(clip_grad_norm_ scales the gradients in place, so the torch arms' gradients have norm 1 after their first tail; the
tail arms leave gradients alone.  Timing does not depend on the values.)

The arms alternate --runs times in one process on one device.  Each block starts from the same weights with a fresh
optimizer and scheduler, runs --warmup untimed tails (the graph arm captures after them), then
  * --iters tails with a device event pair around each: the time the device spends per tail, and
  * --iters tails back to back between two host clock readings, the second after a synchronise: host + device per tail.
Reports per arm the median over all blocks and the median of each block for both clocks (the spread of an arm's block
medians is what a difference between two arms has to exceed), one JSON line per arm plus a summary line; --out also
writes them to a file (profiles/retrieval_optim_tail.txt holds a run; arms are compared within one run only).

--count runs warmup + iters tails of the chosen arms and nothing else: for a kernel trace in a run of its own, to count
launches per tail by differencing two --iters values (the method of profiles/retrieval_train_step_norm.txt, section 2).

    python tools/bench_optim_tail.py [--runs 5] [--warmup 3] [--iters 20] [--arms A,B] [--count] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rq-vae-recommender_amd")]

import torch  # noqa: E402

from modules.model import EncoderDecoderRetrievalModel  # noqa: E402
from modules.scheduler.inv_sqrt import InverseSquareRootScheduler  # noqa: E402
from rqhip.optim import FlatAdamW  # noqa: E402

ARMS = ("torch_foreach", "torch_fused", "tail_eager", "tail_graph")
MAX_NORM, LR, WARMUP_STEPS = 1.0, 1e-3, 10000


class Tail:
    """One arm's optimizer, scheduler and `run()` = one tail, on `params` (gradients already set)."""

    def __init__(self, arm, params, warmup):
        self.params = params
        if arm.startswith("torch"):
            self.opt = torch.optim.AdamW(params, lr=LR, **({"foreach": True} if arm == "torch_foreach" else {"fused": True}))
        else:
            self.opt = FlatAdamW(params, lr=LR, max_grad_norm=MAX_NORM)
        self.sched = InverseSquareRootScheduler(optimizer=self.opt, warmup_steps=WARMUP_STEPS)
        self.graph = None
        self.run = self._torch if arm.startswith("torch") else self._tail
        for _ in range(warmup):
            self.run()
        if arm == "tail_graph":
            # (the warm-up tails ran eagerly on this stream: state, workspace and argument cache exist before the capture)
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.opt.step()
            self.run = self._replay

    def _torch(self):
        torch.nn.utils.clip_grad_norm_(self.params, MAX_NORM)
        self.opt.step()
        self.sched.step()

    def _tail(self):
        self.opt.step()
        self.sched.step()

    def _replay(self):
        self.graph.replay()
        self.sched.step()


def block(arm, params, state, grads, warmup, iters, count_only):
    """One block of one arm from the common starting weights -> (device ms per tail, host-clock ms per tail)."""
    with torch.no_grad():
        for p, w in zip(params, state):
            p.copy_(w)
    for p, g in zip(params, grads):
        p.grad = None if g is None else g.clone()
    tail = Tail(arm, params, warmup)
    torch.cuda.synchronize()
    if count_only:
        for _ in range(iters):
            tail.run()
        torch.cuda.synchronize()
        return [], 0.0
    ms = []
    for _ in range(iters):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        tail.run()
        stop.record()
        stop.synchronize()
        ms.append(start.elapsed_time(stop))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        tail.run()
    torch.cuda.synchronize()
    host_ms = (time.perf_counter() - t0) * 1e3 / iters
    return ms, host_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--arms", default=",".join(ARMS), help="comma-separated subset of: " + ", ".join(ARMS))
    ap.add_argument("--count", action="store_true", help="only run warmup + iters tails per arm and block (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    arms = args.arms.split(",")
    if not arms or any(a not in ARMS for a in arms):
        ap.error(f"--arms takes names from {list(ARMS)}")
    dev = torch.device("cuda")
    torch.manual_seed(5)
    corpus = torch.randint(0, 256, (12101, 3))
    model = EncoderDecoderRetrievalModel(corpus, 3, 256, t5_d_model=384, t5_num_heads=6, t5_d_ff=1024, t5_num_layers=4).to(dev)
    named = list(model.named_parameters())
    params = [p for _, p in named]
    state = [p.detach().clone() for p in params]
    g = torch.Generator(device=dev).manual_seed(6)
    grads = [None if name == "t5_decoder.embed_tokens.weight" else torch.randn(p.shape, generator=g, device=dev) * 1e-2
             for name, p in named]
    n_grad = sum(x is not None for x in grads)
    if args.count:
        for arm in arms:
            block(arm, params, state, grads, args.warmup, args.iters, True)
        print(json.dumps({"count": True, "arms": arms, "tails_per_arm": args.warmup + args.iters, "tensors_with_gradients": n_grad}))
        return
    dev_ms = {a: [] for a in arms}
    dev_blocks = {a: [] for a in arms}
    host_blocks = {a: [] for a in arms}
    for _ in range(args.runs):
        for arm in arms:
            ms, host_ms = block(arm, params, state, grads, args.warmup, args.iters, False)
            dev_ms[arm] += ms
            dev_blocks[arm].append(round(statistics.median(ms), 4))
            host_blocks[arm].append(round(host_ms, 4))
    lines = []
    for arm in arms:
        lines.append(json.dumps({"arm": arm, "tails_timed_per_clock": len(dev_ms[arm]),
                                 "device_event_ms_per_tail_median": round(statistics.median(dev_ms[arm]), 4),
                                 "device_event_ms_per_tail_min": round(min(dev_ms[arm]), 4),
                                 "device_event_block_medians": dev_blocks[arm],
                                 "host_clock_ms_per_tail_median": round(statistics.median(host_blocks[arm]), 4),
                                 "host_clock_ms_per_tail_blocks": host_blocks[arm]}))
    lines.append(json.dumps({"summary": "the optimizer tail alone", "tensors": len(params), "tensors_with_gradients": n_grad,
                             "parameters": sum(p.numel() for p in params), "max_norm": MAX_NORM,
                             "device": torch.cuda.get_device_name(0), "runs": args.runs, "warmup": args.warmup, "iters": args.iters}))
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
