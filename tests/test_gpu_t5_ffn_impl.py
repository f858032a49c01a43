"""ffn_impl = "hip" on the T5 stacks and the retrieval model (modules/t5.py, modules/model.py): the feed-forward body of
every block as one autograd.T5FFNFunction call (csrc/t5_ffn.hip), under every attention_impl / norm_impl.

A small model (d_model 64, 2 heads, d_ff 96, 2 layers, K = 16, L = 3, batch 3; encoder T = 9 with one padded row,
decoder T = 4) against the same module in fp64 on the CPU.  Gates as in tests/test_gpu_t5_ffn.py: e = max|a - a64| /
max|a64| per tensor, e_hip <= max(4 e_torch, 2^-22) for the loss, max(8 e_torch, 2^-22) for parameter gradients, e_torch
from ffn_impl = "torch" with the same attention and norm implementation on the same device."""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

LAYERS = 2
FLOOR = 2.0 ** -22


@functools.lru_cache(maxsize=None)
def _setup():
    """(fp32 model on the device, its fp64 copy on the CPU, the batch on both) -- built once."""
    from data.schemas import TokenizedSeqBatch
    from modules.model import EncoderDecoderRetrievalModel
    B, items, L, K, N = 3, 2, 3, 16, 200
    g = torch.Generator().manual_seed(12)
    torch.manual_seed(12)
    corpus = torch.randint(0, K, (N, L), generator=g)
    model = EncoderDecoderRetrievalModel(corpus, L, K, t5_d_model=64, t5_num_heads=2, t5_d_ff=96, t5_num_layers=LAYERS)
    hist = torch.cat([corpus[torch.randint(0, N, (B, items), generator=g)], torch.zeros(B, items, 1, dtype=torch.long)],
                     dim=-1)
    mask = torch.ones(B, items, L + 1, dtype=torch.bool)
    hist[1, items - 1:] = -1                   # one padded row
    mask[1, items - 1:] = False
    fut = torch.cat([corpus[torch.randint(0, N, (B,), generator=g)], torch.zeros(B, 1, dtype=torch.long)], dim=-1)
    batch = TokenizedSeqBatch(torch.randint(0, 100, (B, 1), generator=g), hist.reshape(B, -1), fut, mask.reshape(B, -1),
                              None, None)
    model64 = copy.deepcopy(model).double().eval()
    dev = torch.device("cuda")
    return (model.to(dev).eval(), model64, TokenizedSeqBatch(*[None if t is None else t.to(dev) for t in batch]), batch)


def _err(a, a64):
    return float((a.double().cpu() - a64).abs().max() / a64.abs().max())


def _gate(name, got, ref32, ref64, factor):
    assert torch.isfinite(got).all(), name
    if not bool(ref64.any()):
        assert not bool(got.any()), name
        return
    e_hip, e_torch = _err(got, ref64), _err(ref32, ref64)
    ratio = e_hip / e_torch if e_torch > 0 else (0.0 if e_hip == 0 else float("inf"))
    print(f"{name}: e_hip {e_hip:.3e} e_torch {e_torch:.3e} ratio {ratio:.2f}")
    assert e_hip <= max(factor * e_torch, FLOOR), name


def _loss_and_grads(model, batch, seed=None):
    model.zero_grad(set_to_none=True)
    if seed is not None:
        torch.manual_seed(seed)
    loss = model(batch).loss
    loss.backward()
    return loss.detach(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


@functools.lru_cache(maxsize=None)
def _reference():
    _, model64, _, batch = _setup()
    return _loss_and_grads(model64, batch)


def _set(model, attention, norm, ffn):
    model.attention_impl, model.norm_impl, model.ffn_impl = attention, norm, ffn
    model._push_attention_impl()


@pytest.mark.parametrize("norm", ["torch", "hip"])
@pytest.mark.parametrize("attention", ["torch", "hip_train"])
def test_eval_loss_and_gradients_against_fp64(attention, norm):
    model, _, batch, _ = _setup()
    loss64, grads64 = _reference()
    _set(model.eval(), attention, norm, "torch")
    loss32, grads32 = _loss_and_grads(model, batch)
    _set(model, attention, norm, "hip")
    loss, grads = _loss_and_grads(model, batch)
    _set(model, "torch", "torch", "torch")
    assert sorted(grads) == sorted(grads64) == sorted(grads32) and len(grads) > 40
    _gate(f"{attention}/{norm} loss", loss.reshape(1), loss32.reshape(1), loss64.reshape(1), 4)
    for n in sorted(grads):
        _gate(f"{attention}/{norm} grad {n}", grads[n], grads32[n], grads64[n], 8)


@pytest.mark.parametrize("attention,norm", [("torch", "torch"), ("hip_train", "torch"), ("torch", "hip"), ("hip_train", "hip")])
def test_train_mode_replays_under_a_seed(attention, norm):
    model, _, batch, _ = _setup()
    _set(model.train(), attention, norm, "hip")
    try:
        loss_a, grads_a = _loss_and_grads(model, batch, seed=5)
        loss_b, grads_b = _loss_and_grads(model, batch, seed=5)
        loss_c, _ = _loss_and_grads(model, batch, seed=6)
    finally:
        _set(model.eval(), "torch", "torch", "torch")
    assert torch.isfinite(loss_a) and torch.equal(loss_a.view(torch.int32), loss_b.view(torch.int32))
    assert sorted(grads_a) == sorted(grads_b) and len(grads_a) > 40
    for n in grads_a:
        assert torch.equal(grads_a[n].view(torch.int32), grads_b[n].view(torch.int32)), n
    assert not torch.equal(loss_a, loss_c)


def _count(monkeypatch, t5):
    calls = {"fwd": 0, "bwd": 0, "randint": 0, "need_h": []}
    o_f, o_b, o_r = t5.ops.t5_ffn_fwd, t5.ops.t5_ffn_bwd, torch.randint

    def fwd(*a, need_h=True, **kw):
        calls["fwd"] += 1
        calls["need_h"].append(need_h)
        out = o_f(*a, need_h=need_h, **kw)
        assert (out[1] is not None) == need_h
        return out

    def bwd(*a, **kw):
        calls["bwd"] += 1
        return o_b(*a, **kw)

    def randint(*a, **kw):
        calls["randint"] += 1
        return o_r(*a, **kw)

    monkeypatch.setattr(t5.ops, "t5_ffn_fwd", fwd)
    monkeypatch.setattr(t5.ops, "t5_ffn_bwd", bwd)
    monkeypatch.setattr(torch, "randint", randint)
    return calls


def _counts(calls):
    return {k: calls[k] for k in ("fwd", "bwd", "randint")}


def test_call_counts(monkeypatch):
    import modules.t5 as t5
    model = _setup()[0]
    enc, dec = model.encoder.encoder, model.t5_decoder
    dev = torch.device("cuda")
    x = torch.randn(3, 9, 64, device=dev)
    memory = torch.randn(3, 9, 64, device=dev)
    y = torch.randn(3, 4, 64, device=dev)
    calls = _count(monkeypatch, t5)

    def reset():
        calls.update(fwd=0, bwd=0, randint=0, need_h=[])

    try:
        for norm in ("torch", "hip"):
            for stack in (enc, dec):
                stack.attention_impl, stack.norm_impl, stack.ffn_impl = "torch", norm, "torch"
            model.eval()
            enc(x), dec(y, encoder_hidden_states=memory)
            model.train()
            enc(x).sum().backward()
            assert calls["fwd"] == 0 and calls["bwd"] == 0     # "torch": the fused op is never called
            assert calls["randint"] == (1 if norm == "hip" else 0)
            reset()
        for norm in ("torch", "hip"):
            for stack in (enc, dec):
                stack.attention_impl, stack.norm_impl, stack.ffn_impl = "torch", norm, "hip"
            # eval mode under grad: one Function call per block, no seeds
            model.eval()
            enc(x).sum().backward()
            assert _counts(calls) == {"fwd": LAYERS, "bwd": LAYERS, "randint": 0} and all(calls["need_h"])
            reset()
            dec(y, encoder_hidden_states=memory).sum().backward()
            assert _counts(calls) == {"fwd": LAYERS, "bwd": LAYERS, "randint": 0}
            reset()
            # under no_grad no h is allocated
            with torch.no_grad():
                enc(x), dec(y, encoder_hidden_states=memory)
            assert _counts(calls) == {"fwd": 2 * LAYERS, "bwd": 0, "randint": 0} and not any(calls["need_h"])
            reset()
            # train mode: norm "hip" keeps its one draw per stack forward, norm "torch" draws one seed per feed-forward
            model.train()
            draws = 1 if norm == "hip" else LAYERS
            enc(x).sum().backward()
            assert _counts(calls) == {"fwd": LAYERS, "bwd": LAYERS, "randint": draws}
            reset()
            dec(y, encoder_hidden_states=memory).sum().backward()
            assert _counts(calls) == {"fwd": LAYERS, "bwd": LAYERS, "randint": draws}
            reset()
            with torch.no_grad():
                enc(x)
            assert _counts(calls) == {"fwd": LAYERS, "bwd": 0, "randint": draws} and not any(calls["need_h"])
            reset()
    finally:
        model.eval()
        model.zero_grad(set_to_none=True)
        for stack in (enc, dec):
            stack.attention_impl, stack.norm_impl, stack.ffn_impl = "torch", "torch", "torch"


@pytest.mark.parametrize("attention", ["torch", "hip"])
def test_generate_runs_with_hip_ffn(attention):
    model, _, batch, _ = _setup()
    _set(model.eval(), attention, "torch", "hip")
    torch.manual_seed(1)
    out = model.generate_next_sem_id(batch)
    _set(model, "torch", "torch", "torch")
    ids, scores = out.sem_ids, out.log_probas
    assert ids.shape == (3, 10, 3) and scores.shape == (3, 10) and not bool(torch.isnan(scores).any())
    valid = scores != float("-inf")
    assert bool(valid.any(dim=1).all()) and bool(torch.isfinite(scores[valid]).all())
    corpus = model.codebooks.to(ids.device)
    assert bool((ids[valid][:, None, :] == corpus[None]).all(-1).any(-1).all())     # a valid beam is a corpus row


def test_unsupported_d_ff_runs_the_operators(monkeypatch):
    import modules.t5 as t5
    from modules.t5 import T5Config, T5Stack
    dev = torch.device("cuda")
    torch.manual_seed(2)
    stack = T5Stack(T5Config(16, d_model=64, num_heads=1, d_ff=40, num_layers=1)).to(dev).eval()
    x = torch.randn(2, 5, 64, device=dev)
    calls = _count(monkeypatch, t5)
    with torch.no_grad():
        want = stack(x)
        stack.ffn_impl = "hip"
        got = stack(x)
    assert calls["fwd"] == 0 and torch.equal(got, want)
