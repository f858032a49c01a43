"""norm_impl = "hip" on the T5 stacks and the retrieval model (modules/t5.py, modules/model.py): every dropout, residual
add and RMS norm between two sub-layer bodies as one autograd.T5AddNormFunction call (csrc/t5_add_norm.hip).

A small model (d_model 64, 2 heads, d_ff 128, 2 layers, K = 16, L = 3, batch 3; encoder T = 9 with one padded row,
decoder T = 4) against the same module in fp64 on the CPU.  Gates: retrieval_cases.gate, e = max|a - a64| /
max|a64| per tensor, e_kernel <= max(4 e_torch, 2^-22) for the loss and hidden states, max(8 e_torch, 2^-22) for parameter
gradients, e_torch from norm_impl = "torch" with the same attention implementation on the same device."""
import pytest
import torch

from retrieval_cases import LAYERS, gate, impls, loss_and_grads, reference, same_bits, small_model

pytestmark = pytest.mark.gpu

SMALL = (11, 128, True)         # retrieval_cases.small_model: seed, d_ff, norm weights perturbed


@pytest.mark.parametrize("attention", ["torch", "hip_train"])
def test_eval_loss_and_gradients_against_fp64(attention):
    model, _, batch, _ = small_model(*SMALL)
    loss64, grads64 = reference(*SMALL)
    with impls(model.eval(), attention=attention):
        loss32, grads32 = loss_and_grads(model, batch)
    with impls(model, attention=attention, norm="hip"):
        loss, grads = loss_and_grads(model, batch)
    assert sorted(grads) == sorted(grads64) == sorted(grads32) and len(grads) > 40
    gate(f"{attention} loss", loss.reshape(1), loss32.reshape(1), loss64.reshape(1), 4)
    for n in sorted(grads):
        gate(f"{attention} grad {n}", grads[n], grads32[n], grads64[n], 8)


def _decoder_inputs():
    model, model64, batch, batch_cpu = small_model(*SMALL)
    from modules.model import _strip_dedup_col
    L = model.num_hierarchies
    with torch.no_grad():
        enc64, mask = model64.encoder_forward_pass(_strip_dedup_col(batch_cpu.seq_mask.long(), L + 1, L),
                                                   _strip_dedup_col(batch_cpu.sem_ids, L + 1, L), batch_cpu.user_ids)
        x64 = torch.randn(3, 4, 64, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
        hidden64 = model64.t5_decoder(x64, encoder_hidden_states=enc64, encoder_attention_mask=mask)
    dev = torch.device("cuda")
    return x64.float().to(dev), enc64.float().to(dev), mask.to(dev), hidden64


def _decode(dec, path, x, enc, mask):
    """The decoder's hidden states [R, T, d] of the T positions of x on one of the three inference paths."""
    R, T = x.shape[0], x.shape[1]
    with torch.no_grad():
        if path == "operators, past_key_values":
            dec.attention_impl = "torch"
            cross_kv, past, out = dec.cross_kv(enc), None, []
            for t in range(T):
                h, past = dec(x[:, t:t + 1], encoder_attention_mask=mask, past_key_values=past, use_cache=True,
                              cross_kv=cross_kv)
                out.append(h)
            return torch.cat(out, dim=1)
        dec.attention_impl = "hip"
        if path == "hip, no cache":
            return dec(x, encoder_hidden_states=enc, encoder_attention_mask=mask)
        cache, cross_kv, out = dec.new_decode_cache(T, R, x.device), dec.cross_kv(enc), []
        for t in range(T):
            if t:
                cache.reorder(torch.arange(R, device=x.device))
            out.append(dec(x[:, t:t + 1], encoder_attention_mask=mask, cross_kv=cross_kv, decode_cache=cache))
        return torch.cat(out, dim=1)


@pytest.mark.parametrize("path", ["operators, past_key_values", "hip, no cache", "hip, decode_cache"])
def test_decoder_hidden_states_without_grad(path, monkeypatch):
    import modules.t5 as t5
    model = small_model(*SMALL)[0].eval()
    dec = model.t5_decoder
    x, enc, mask, hidden64 = _decoder_inputs()
    calls = _count(monkeypatch, t5)
    with impls(model):                     # the decoder stack is set directly; the exit resets it
        ref32 = _decode(dec, path, x, enc, mask)
        assert calls["fwd"] == 0
        dec.norm_impl = "hip"
        got = _decode(dec, path, x, enc, mask)
    steps = 1 if path == "hip, no cache" else x.shape[1]
    assert calls["fwd"] == steps * (3 * LAYERS + 1)
    gate(f"decoder hidden states, {path}", got, ref32, hidden64, 4)


@pytest.mark.parametrize("attention", ["torch", "hip"])
def test_generate_runs_with_hip_norm(attention):
    model, _, batch, _ = small_model(*SMALL)
    with impls(model.eval(), attention=attention, norm="hip"):
        torch.manual_seed(1)
        out = model.generate_next_sem_id(batch)
    ids, scores = out.sem_ids, out.log_probas
    assert ids.shape == (3, 10, 3) and scores.shape == (3, 10) and not bool(torch.isnan(scores).any())
    valid = scores != float("-inf")
    assert bool(valid.any(dim=1).all()) and bool(torch.isfinite(scores[valid]).all())
    corpus = model.codebooks.to(ids.device)
    assert bool((ids[valid][:, None, :] == corpus[None]).all(-1).any(-1).all())     # a valid beam is a corpus row


@pytest.mark.parametrize("attention", ["torch", "hip_train"])
def test_train_mode_replays_under_a_seed(attention):
    model, _, batch, _ = small_model(*SMALL)
    with impls(model.eval(), attention=attention, norm="hip"):
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
    calls = {"fwd": 0, "bwd": 0, "randint": 0}
    o_f, o_b, o_r = t5.ops.t5_add_norm_fwd, t5.ops.t5_add_norm_bwd, torch.randint

    def fwd(*a, **kw):
        calls["fwd"] += 1
        return o_f(*a, **kw)

    def bwd(*a, **kw):
        calls["bwd"] += 1
        return o_b(*a, **kw)

    def randint(*a, **kw):
        calls["randint"] += 1
        return o_r(*a, **kw)

    monkeypatch.setattr(t5.ops, "t5_add_norm_fwd", fwd)
    monkeypatch.setattr(t5.ops, "t5_add_norm_bwd", bwd)
    monkeypatch.setattr(torch, "randint", randint)
    return calls


def test_call_counts(monkeypatch):
    import modules.t5 as t5
    model = small_model(*SMALL)[0]
    enc, dec = model.encoder.encoder, model.t5_decoder
    dev = torch.device("cuda")
    x = torch.randn(3, 9, 64, device=dev)
    memory = torch.randn(3, 9, 64, device=dev)
    y = torch.randn(3, 4, 64, device=dev)
    calls = _count(monkeypatch, t5)
    with impls(model.eval()):
        enc(x), dec(y, encoder_hidden_states=memory)
        model.train()
        enc(x).sum().backward()
        assert calls == {"fwd": 0, "bwd": 0, "randint": 0}      # "torch": the fused op is never called
    with impls(model, norm="hip"):
        enc(x)
        assert calls == {"fwd": 2 * LAYERS + 1, "bwd": 0, "randint": 0}
        dec(y, encoder_hidden_states=memory)
        assert calls == {"fwd": 5 * LAYERS + 2, "bwd": 0, "randint": 0}
        # train mode: one draw of seeds per stack forward, one backward call per forward call
        model.train()
        calls.update(fwd=0)
        enc(x).sum().backward()
        assert calls == {"fwd": 2 * LAYERS + 1, "bwd": 2 * LAYERS + 1, "randint": 1}
        calls.update(fwd=0, bwd=0, randint=0)
        dec(y, encoder_hidden_states=memory).sum().backward()
        assert calls == {"fwd": 3 * LAYERS + 1, "bwd": 3 * LAYERS + 1, "randint": 1}
        # the fused attention draws its own seed per call; add-norm adds one draw, not one per call
        enc.attention_impl = "hip_train"
        calls.update(fwd=0, bwd=0, randint=0)
        enc(x).sum().backward()
        assert calls == {"fwd": 2 * LAYERS + 1, "bwd": 2 * LAYERS + 1, "randint": LAYERS + 1}


def test_unsupported_width_runs_the_operators(monkeypatch):
    import modules.t5 as t5
    from modules.t5 import T5Config, T5Stack
    dev = torch.device("cuda")
    torch.manual_seed(2)
    stack = T5Stack(T5Config(16, d_model=66, num_heads=1, d_ff=32, num_layers=1)).to(dev).eval()
    x = torch.randn(2, 5, 66, device=dev)
    calls = _count(monkeypatch, t5)
    with torch.no_grad():
        want = stack(x)
        stack.norm_impl = "hip"
        got = stack(x)
    assert calls["fwd"] == 0 and torch.equal(got, want)
