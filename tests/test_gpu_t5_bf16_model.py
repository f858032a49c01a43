"""`matmul_arith = "bf16"` on the retrieval model, on the GPU: which entry points a forward, a backward and a generate
reach, gradients, the generated ids, the loss against the fp32 arm, and train_decoder.train with amp.

The model is retrieval_cases.tiny_model at the smallest widths the kernels take (d_model 32, d_ff 32; one block per
stack, 2 heads of 64).

Loss agreement.  The bf16 arm rounds every operand of the feed-forward and projection products to 8 significant bits, so
its loss differs from the fp32 arm's by a small multiple of 2^-9 per product, damped by the norms and the softmax; how
much is measured, not derived: |loss_bf16 - loss_fp32| / |loss_fp32| on the same weights and batch in train mode, over
the 8 seeds 0 .. 7 (batch and dropout).  The threshold LOSS_TOL is 4 times the largest value observed on an MI355X
(1.718e-4 at seed 0; the seeds are a small sample) and may not exceed 2^-6; the eight values and the threshold:
profiles/t5_bf16_error.txt."""
import pytest
import torch

from retrieval_cases import loss_and_grads, same_bits, tiny_model, to_device

pytestmark = pytest.mark.gpu

LOSS_SEEDS = range(8)
LOSS_TOL = 4 * 1.718e-4     # 6.872e-4: 4 x the largest measured relative difference (docstring); never above 2^-6
OPS = ("t5_ffn_fwd", "t5_ffn_bwd", "t5_proj_fwd", "t5_proj_bwd")


def _model(dev):
    m = tiny_model(32, 32).to(dev)
    m.attention_impl, m.norm_impl, m.head_impl = "hip_train", "hip", "hip"
    m.ffn_impl, m.proj_impl = "hip", "hip"
    return m


def _batch(seed, dev, B=2):
    from data.schemas import TokenizedSeqBatch
    g = torch.Generator().manual_seed(seed)
    return to_device(TokenizedSeqBatch(torch.zeros(B, 1, dtype=torch.long), torch.randint(0, 16, (B, 8), generator=g),
                                       torch.randint(0, 16, (B, 4), generator=g), torch.ones(B, 8, dtype=torch.bool),
                                       None, None), dev)


def _count(monkeypatch):
    """Every call of the four ops, by the arithmetic it asks for."""
    import modules.t5 as t5
    calls = {name: {"fp32": 0, "bf16": 0} for name in OPS}
    for name in OPS:
        def counted(*a, _name=name, _real=getattr(t5.ops, name), **kw):
            arith = kw.get("arith", "fp32")
            assert arith in ("fp32", "bf16"), arith
            calls[_name][arith] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(t5.ops, name, counted)
    return calls


def _total(calls, arith):
    return {name: c[arith] for name, c in calls.items()}


def test_every_call_takes_the_chosen_arm(monkeypatch):
    dev = torch.device("cuda")
    model, batch = _model(dev).eval(), _batch(1, dev)
    plain, _ = loss_and_grads(model, batch)                      # before anything touches the attribute
    calls = _count(monkeypatch)
    model.matmul_arith = "fp32"
    loss32, grads32 = loss_and_grads(model, batch)
    model.generate_next_sem_id(batch)
    n32 = _total(calls, "fp32")
    assert same_bits(loss32, plain) and all(v == 0 for v in _total(calls, "bf16").values())
    assert n32["t5_ffn_fwd"] > 0 and n32["t5_ffn_bwd"] > 0 and n32["t5_proj_fwd"] > 0 and n32["t5_proj_bwd"] > 0
    for c in calls.values():
        c.update(fp32=0, bf16=0)
    model.matmul_arith = "bf16"
    loss16, grads16 = loss_and_grads(model, batch)
    out = model.generate_next_sem_id(batch)
    # the same calls, every one of them on the other arm: feed-forward, q / k / v / o, the cross-attention K/V and the
    # decode steps' slab writes
    assert _total(calls, "bf16") == n32 and all(v == 0 for v in _total(calls, "fp32").values())
    assert torch.isfinite(loss16) and not same_bits(loss16, loss32)
    names = [n for n, _ in model.named_parameters()]
    assert sorted(grads16) == sorted(grads32)
    for n in names:
        if n in grads32:
            assert torch.isfinite(grads16[n]).all(), n
    used = [n for n in names if n in grads16]
    assert len(used) > 20 and any(".wi." in n for n in used) and any(".q." in n for n in used)
    # generate: every beam with a finite score is a row of the corpus
    corpus = {tuple(r) for r in model.codebooks.tolist()}
    ids, lp = out.sem_ids, out.log_probas
    assert ids.shape[0] == 2 and ids.shape[-1] == model.num_hierarchies
    assert bool(torch.isfinite(lp[:, 0]).all())
    for b in range(ids.shape[0]):
        for k in range(ids.shape[1]):
            if bool(torch.isfinite(lp[b, k])):
                assert tuple(ids[b, k].tolist()) in corpus, (b, k)
    # under no_grad the forward takes the arm too
    for c in calls.values():
        c.update(fp32=0, bf16=0)
    with torch.no_grad():
        loss_n = model(batch).loss
    assert calls["t5_ffn_fwd"]["bf16"] > 0 and calls["t5_proj_fwd"]["bf16"] > 0
    assert all(v == 0 for v in _total(calls, "fp32").values()) and same_bits(loss_n, loss16)


def test_every_parameter_gets_a_finite_gradient_in_train_mode():
    """Every parameter the fp32 arm gives a gradient (all but the tables no forward reads) gets a finite one."""
    dev = torch.device("cuda")
    model, batch = _model(dev).train(), _batch(2, dev)
    model.matmul_arith = "bf16"
    want = sorted(n for n, _ in model.named_parameters())
    model.matmul_arith = "fp32"
    _, grads32 = loss_and_grads(model, batch, seed=5)
    model.matmul_arith = "bf16"
    loss, grads = loss_and_grads(model, batch, seed=5)
    assert torch.isfinite(loss) and sorted(grads) == sorted(grads32) and set(grads) <= set(want)
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    again, grads2 = loss_and_grads(model, batch, seed=5)             # the same seeds: the same bits
    assert same_bits(loss, again) and all(same_bits(grads[n], grads2[n]) for n in grads)


def test_loss_agrees_with_the_fp32_arm():
    dev = torch.device("cuda")
    model = _model(dev).train()
    rel = []
    for s in LOSS_SEEDS:
        batch = _batch(100 + s, dev, B=8)
        losses = {}
        for arith in ("fp32", "bf16"):
            model.matmul_arith = arith
            torch.manual_seed(s)                                     # the same dropout seeds on both arms
            losses[arith] = float(model(batch).loss.detach())       # under grad: the path a training step takes
        rel.append(abs(losses["bf16"] - losses["fp32"]) / abs(losses["fp32"]))
        print(f"loss seed {s}: fp32 {losses['fp32']:.7f} bf16 {losses['bf16']:.7f} relative difference {rel[-1]:.3e}")
    print(f"loss: largest relative difference {max(rel):.3e}, threshold {LOSS_TOL:.3e}")
    assert LOSS_TOL <= 2.0 ** -6 and 0 < max(rel) <= LOSS_TOL


def test_train_decoder_with_amp_bf16(tmp_path, monkeypatch):
    import os

    import train_decoder
    from test_gpu_train_decoder import _config
    calls = _count(monkeypatch)
    root = str(tmp_path) + "/"
    torch.manual_seed(0)
    out = train_decoder.train(**_config(save_dir_root=root, iterations=4, partial_eval_every=100, full_eval_every=100,
                                        amp=True, mixed_precision_type="bf16"))
    assert [it for it, _ in out["losses"]] == [0, 1, 2, 3]
    assert all(torch.isfinite(torch.tensor(v)) for _, v in out["losses"])
    assert out["checkpoint"] == root + "checkpoint_3.pt" and os.path.exists(out["checkpoint"])
    # the feed-forward ran on the bf16 arm, forward and backward; train leaves the projections to the operators
    per = 2 * 2                                  # feed-forward bodies per step: t5_num_layers in each of the two stacks
    assert calls["t5_ffn_fwd"] == {"fp32": 0, "bf16": 4 * per} and calls["t5_ffn_bwd"] == {"fp32": 0, "bf16": 4 * per}
    assert calls["t5_proj_fwd"] == {"fp32": 0, "bf16": 0}
    state = torch.load(out["checkpoint"], map_location="cpu", weights_only=False)
    assert all(v.dtype != torch.bfloat16 for v in state["model"].values())
    # a default run resumes from it: the state dict is the fp32 arm's
    torch.manual_seed(0)
    more = train_decoder.train(**_config(save_dir_root=root + "next/", pretrained_decoder_path=out["checkpoint"],
                                         iterations=1, partial_eval_every=100, full_eval_every=100))
    assert (more["start_iter"], more["end_iter"]) == (4, 5) and torch.isfinite(torch.tensor(more["losses"][0][1]))
    assert calls["t5_ffn_fwd"] == {"fp32": per, "bf16": 4 * per}
