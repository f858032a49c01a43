"""ffn_impl = "hip" on the T5 stacks and the retrieval model (modules/t5.py, modules/model.py): the feed-forward body of
every block as one autograd.T5FFNFunction call (csrc/t5_ffn.hip), under every attention_impl / norm_impl.

A small model (d_model 64, 2 heads, d_ff 96, 2 layers, K = 16, L = 3, batch 3; encoder T = 9 with one padded row,
decoder T = 4) against the same module in fp64 on the CPU.  Gates: retrieval_cases.gate, e = max|a - a64| /
max|a64| per tensor, e_kernel <= max(4 e_torch, 2^-22) for the loss, max(8 e_torch, 2^-22) for parameter gradients, e_torch
from ffn_impl = "torch" with the same attention and norm implementation on the same device."""
import pytest
import torch

from retrieval_cases import LAYERS, gate, impls, loss_and_grads, reference, same_bits, small_model

pytestmark = pytest.mark.gpu

SMALL = (12, 96, False)         # retrieval_cases.small_model: seed, d_ff, norm weights as initialised


@pytest.mark.parametrize("norm", ["torch", "hip"])
@pytest.mark.parametrize("attention", ["torch", "hip_train"])
def test_eval_loss_and_gradients_against_fp64(attention, norm):
    model, _, batch, _ = small_model(*SMALL)
    loss64, grads64 = reference(*SMALL)
    with impls(model.eval(), attention=attention, norm=norm):
        loss32, grads32 = loss_and_grads(model, batch)
    with impls(model, attention=attention, norm=norm, ffn="hip"):
        loss, grads = loss_and_grads(model, batch)
    assert sorted(grads) == sorted(grads64) == sorted(grads32) and len(grads) > 40
    gate(f"{attention}/{norm} loss", loss.reshape(1), loss32.reshape(1), loss64.reshape(1), 4)
    for n in sorted(grads):
        gate(f"{attention}/{norm} grad {n}", grads[n], grads32[n], grads64[n], 8)


@pytest.mark.parametrize("attention,norm", [("torch", "torch"), ("hip_train", "torch"), ("torch", "hip"), ("hip_train", "hip")])
def test_train_mode_replays_under_a_seed(attention, norm):
    model, _, batch, _ = small_model(*SMALL)
    with impls(model.eval(), attention=attention, norm=norm, ffn="hip"):
        model.train()
        loss_a, grads_a = loss_and_grads(model, batch, seed=5)
        loss_b, grads_b = loss_and_grads(model, batch, seed=5)
        loss_c, _ = loss_and_grads(model, batch, seed=6)
    assert torch.isfinite(loss_a) and same_bits(loss_a, loss_b)
    assert sorted(grads_a) == sorted(grads_b) and len(grads_a) > 40
    for n in grads_a:
        assert same_bits(grads_a[n], grads_b[n]), n
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
    model = small_model(*SMALL)[0]
    enc, dec = model.encoder.encoder, model.t5_decoder
    dev = torch.device("cuda")
    x = torch.randn(3, 9, 64, device=dev)
    memory = torch.randn(3, 9, 64, device=dev)
    y = torch.randn(3, 4, 64, device=dev)
    calls = _count(monkeypatch, t5)

    def reset():
        calls.update(fwd=0, bwd=0, randint=0, need_h=[])

    for norm in ("torch", "hip"):
        with impls(model.eval(), norm=norm):
            enc(x), dec(y, encoder_hidden_states=memory)
            model.train()
            enc(x).sum().backward()
            assert calls["fwd"] == 0 and calls["bwd"] == 0     # "torch": the fused op is never called
            assert calls["randint"] == (1 if norm == "hip" else 0)
            reset()
    for norm in ("torch", "hip"):
        with impls(model, norm=norm, ffn="hip"):
            # eval mode under grad: one Function call per block, no seeds
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


@pytest.mark.parametrize("attention", ["torch", "hip"])
def test_generate_runs_with_hip_ffn(attention):
    model, _, batch, _ = small_model(*SMALL)
    with impls(model.eval(), attention=attention, ffn="hip"):
        torch.manual_seed(1)
        out = model.generate_next_sem_id(batch)
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
