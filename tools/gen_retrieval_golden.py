#!/usr/bin/env python3
"""Generate tests/golden/retrieval_*.npz by running the reference's retrieval model on CPU.

The reference's modules/model.py (EncoderDecoderRetrievalModel, HuggingFace T5) is imported in place from
RQ_REFERENCE_ROOT (default /root/reference), as oracle/gen_golden.py does for the tokenizer half; nothing is copied
from it.  Needs `transformers`; CPU only; a few seconds.

Per fixture (a, b, c) the file holds the model's weights under their state-dict names (the unused `shared` /
`embed_tokens` tables are left out: the test fills them), a corpus with duplicate and shared-prefix rows, a batch in
the tokenizer's layout (padded -1 history, dedup column), loss / loss_d / every gradient of forward() in eval mode,
and for generate() the Exp(1) noise of each step with the resulting sem_ids and log_probas.

The noise is recorded by replacing torch.multinomial in this process with the exponential race ATen runs for
sampling without replacement (topk(p / q, n), q = empty_like(p).exponential_(1)); the script first asserts that the
replacement returns what torch.multinomial returns under the same seed, for the whole generate() of every fixture.

retrieval_state_dict.npz holds the names and shapes of the default config's state_dict() and its parameter count.

inv_sqrt_sched.npz is recorded from the reference's modules/scheduler/inv_sqrt.py:InverseSquareRootScheduler on a CPU
torch.optim.AdamW (base lr 1e-3, 8 optimizer steps, warm-up 3 and warm-up 1): per case the lr each optimizer step ran at,
get_last_lr() after each scheduler step, and last_epoch / _step_count after the fourth; plus the key names of its state dict.

    python tools/gen_retrieval_golden.py [--sched-only]
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("RQ_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")
MAX_BYTES = 1 << 20

# name: (L, K, d_model, heads, d_ff, layers, sep, user_bins, k, B, items, corpus rows, seed)
CASES = {
    "a": dict(L=3, K=16, d=32, heads=2, d_ff=64, layers=2, sep=True, bins=None, k=10, B=6, items=5, N=40, seed=1),
    "b": dict(L=4, K=8, d=24, heads=3, d_ff=48, layers=1, sep=False, bins=7, k=5, B=5, items=4, N=30, seed=2),
    "c": dict(L=3, K=256, d=32, heads=1, d_ff=64, layers=1, sep=True, bins=None, k=10, B=6, items=5, N=2000, seed=3),
}
UNUSED = ("encoder.shared.weight", "encoder.encoder.embed_tokens.weight", "t5_decoder.embed_tokens.weight")


def import_reference():
    sys.path.insert(0, ROOT)
    from oracle.gen_golden import _install_stubs
    _install_stubs()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from modules import model as m  # noqa
    from data import schemas as sch  # noqa
    return m, sch


def make_corpus(g: torch.Generator, N: int, L: int, K: int) -> torch.Tensor:
    """Random rows, then duplicates of some rows and rows that share all but the last id with another."""
    base = torch.randint(0, K, (N - N // 4, L), generator=g)
    dup = base[torch.randint(0, base.shape[0], (N // 8,), generator=g)]
    sib = base[torch.randint(0, base.shape[0], (N // 4 - N // 8,), generator=g)].clone()
    sib[:, -1] = torch.randint(0, K, (sib.shape[0],), generator=g)
    rows = torch.cat([base, dup, sib])
    return rows[torch.randperm(rows.shape[0], generator=g)]


def make_batch(sch, g: torch.Generator, corpus: torch.Tensor, B: int, items: int, L: int):
    """Histories of corpus items in the tokenizer's layout: L ids + a dedup column per item, -1 and mask False on
    padded items (user b has b % items padded items at the end, at least one item is real)."""
    N = corpus.shape[0]
    pick = torch.randint(0, N, (B, items), generator=g)
    ids = torch.cat([corpus[pick], torch.randint(0, 3, (B, items, 1), generator=g)], dim=-1)  # [B, items, L+1]
    mask = torch.ones(B, items, L + 1, dtype=torch.bool)
    for b in range(B):
        pad = b % items
        if pad:
            ids[b, items - pad:] = -1
            mask[b, items - pad:] = False
    fut = torch.cat([corpus[torch.randint(0, N, (B,), generator=g)], torch.zeros(B, 1, dtype=torch.long)], dim=-1)
    user_ids = torch.randint(0, 1000, (B, 1), generator=g)
    tt = torch.arange(L + 1).repeat(items).expand(B, -1).contiguous()
    return sch.TokenizedSeqBatch(user_ids=user_ids, sem_ids=ids.reshape(B, -1), sem_ids_fut=fut,
                                 seq_mask=mask.reshape(B, -1), token_type_ids=tt,
                                 token_type_ids_fut=torch.arange(L + 1).expand(B, -1).contiguous())


class RecordingMultinomial:
    """torch.multinomial(p, n, replacement=False) as ATen computes it, keeping each Exp(1) draw."""

    def __init__(self):
        self.noise = []
        self.orig = torch.multinomial

    def __call__(self, p, num_samples, replacement=False, generator=None):
        assert not replacement and generator is None
        q = torch.empty_like(p).exponential_(1)
        self.noise.append(q.clone())
        return torch.topk(p / q, num_samples).indices


def gen_case(m, sch, name: str, c: dict) -> None:
    torch.manual_seed(c["seed"])
    g = torch.Generator().manual_seed(100 + c["seed"])
    L, K = c["L"], c["K"]
    corpus = make_corpus(g, c["N"], L, K)
    model = m.EncoderDecoderRetrievalModel(corpus, L, K, t5_d_model=c["d"], t5_num_heads=c["heads"],
                                           t5_d_ff=c["d_ff"], t5_num_layers=c["layers"],
                                           top_k_for_generation=c["k"], should_add_sep_token=c["sep"],
                                           num_user_bins=c["bins"])
    # scale the heads so the softmax is peaked enough for prefix masking and ties to matter
    with torch.no_grad():
        for lin in model.decoder_mlp:
            lin.weight.mul_(8.0)
    batch = make_batch(sch, g, corpus, c["B"], c["items"], L)
    model.eval()
    out = model(batch)
    model.zero_grad()
    out.loss.backward()
    rec = {}
    for k, v in model.state_dict().items():
        if k not in UNUSED:
            rec["w." + k] = v.detach().numpy().copy()
    for k, p in model.named_parameters():
        if p.grad is not None:
            rec["g." + k] = p.grad.detach().numpy().astype(np.float32)
    rec["loss"] = np.float32(out.loss.item())
    rec["loss_d"] = out.loss_d.numpy().astype(np.float32)

    # generate(): the real multinomial and the recording race must agree under the same seed
    torch.manual_seed(1000 + c["seed"])
    ref_ids, ref_lp = model.generate_next_sem_id(batch)
    recorder = RecordingMultinomial()
    torch.multinomial = recorder
    try:
        torch.manual_seed(1000 + c["seed"])
        ids, lp = model.generate_next_sem_id(batch)
    finally:
        torch.multinomial = recorder.orig
    assert torch.equal(ids, ref_ids), f"{name}: recording multinomial differs from torch.multinomial (ids)"
    assert torch.equal(lp, ref_lp), f"{name}: recording multinomial differs from torch.multinomial (log_probas)"
    assert len(recorder.noise) == L
    for h, q in enumerate(recorder.noise):
        rec[f"noise{h}"] = q.numpy().astype(np.float32)
    rec["sem_ids"] = ids.numpy().astype(np.int64)
    rec["log_probas"] = lp.numpy().astype(np.float32)
    n_valid = int(torch.isfinite(lp).sum())

    rec["corpus"] = corpus.numpy().astype(np.int64)
    for f in batch._fields:
        rec["batch." + f] = getattr(batch, f).numpy()
    rec["config"] = np.array([L, K, c["d"], c["heads"], c["d_ff"], c["layers"], int(c["sep"]), c["bins"] or 0, c["k"]],
                             dtype=np.int64)
    path = os.path.join(OUT, f"retrieval_{name}.npz")
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    assert size < MAX_BYTES, (path, size)
    print(f"{path}: {size} bytes, loss {out.loss.item():.6f}, {n_valid}/{lp.numel()} finite beams")


def gen_state_dict(m) -> None:
    torch.manual_seed(0)
    model = m.EncoderDecoderRetrievalModel(torch.zeros(10, 4, dtype=torch.long), 3, 256)
    sd = model.state_dict()
    names = np.array(list(sd.keys()))
    shapes = np.full((len(sd), 2), -1, dtype=np.int64)
    for i, v in enumerate(sd.values()):
        shapes[i, :v.dim()] = v.shape
    n_params = sum(p.numel() for p in model.parameters())
    path = os.path.join(OUT, "retrieval_state_dict.npz")
    np.savez_compressed(path, names=names, shapes=shapes, n_params=np.int64(n_params))
    assert os.path.getsize(path) < MAX_BYTES
    print(f"{path}: {len(names)} entries, {n_params} parameters")


SCHED_CASES = {"w3": dict(base_lr=1e-3, warmup=3, steps=8), "w1": dict(base_lr=1e-3, warmup=1, steps=8)}


def gen_inv_sqrt_sched() -> None:
    """The reference's train_decoder.py loop around its scheduler: optimizer.step(), then lr_scheduler.step()."""
    from modules.scheduler.inv_sqrt import InverseSquareRootScheduler  # (the reference's: REF is first on sys.path)
    assert os.path.abspath(sys.modules[InverseSquareRootScheduler.__module__].__file__).startswith(os.path.abspath(REF))
    rec = {}
    for name, c in SCHED_CASES.items():
        p = torch.nn.Parameter(torch.ones(3))
        opt = torch.optim.AdamW([p], lr=c["base_lr"])
        sched = InverseSquareRootScheduler(optimizer=opt, warmup_steps=c["warmup"])
        used, last = [], []
        for t in range(c["steps"]):
            p.grad = torch.ones(3)
            used.append(opt.param_groups[0]["lr"])
            opt.step()
            sched.step()
            last.append(sched.get_last_lr()[0])
            if t == 3:
                sd = sched.state_dict()
                rec[f"{name}.after4"] = np.array([sd["last_epoch"], sd["_step_count"]], dtype=np.int64)
        rec[f"{name}.lr_used"] = np.array(used, dtype=np.float64)
        rec[f"{name}.last_lr"] = np.array(last, dtype=np.float64)
        rec[f"{name}.config"] = np.array([c["base_lr"], c["warmup"], c["steps"]], dtype=np.float64)
    rec["state_dict_keys"] = np.array(sorted(sched.state_dict().keys()))
    path = os.path.join(OUT, "inv_sqrt_sched.npz")
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) < MAX_BYTES
    print(f"{path}: {os.path.getsize(path)} bytes, keys {list(rec['state_dict_keys'])}, w3 lrs {rec['w3.lr_used']}")


def main() -> None:
    m, sch = import_reference()
    torch.set_num_threads(4)
    gen_inv_sqrt_sched()
    if sys.argv[1:] == ["--sched-only"]:
        return
    gen_state_dict(m)
    for name, c in CASES.items():
        gen_case(m, sch, name, c)


if __name__ == "__main__":
    main()
