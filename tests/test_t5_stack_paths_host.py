"""T5Stack.forward on the operator path (modules/t5.py) against a straight-line restatement from the stack's own
submodules, on the CPU: the values, and in train mode the order in which the dropouts use the generator.

Encoder and decoder of T5Config(16, d_model=32, num_heads=2, d_ff=64, num_layers=2, dropout_rate=0.1); inputs [3, 5, 32],
an encoder output [3, 6, 32], padding masks with one masked key in each."""
import functools

import pytest
import torch

SEED = 11


@functools.lru_cache(maxsize=None)
def _setup():
    from modules.t5 import T5Config, T5Stack
    torch.manual_seed(3)
    stacks = {dec: T5Stack(T5Config(16, d_model=32, num_heads=2, d_ff=64, num_layers=2, dropout_rate=0.1, is_decoder=dec))
              for dec in (False, True)}
    emb, memory = torch.randn(3, 5, 32), torch.randn(3, 6, 32)
    mask, memory_mask = torch.ones(3, 5, dtype=torch.long), torch.ones(3, 6, dtype=torch.long)
    mask[1, 3] = 0
    memory_mask[2, 4:] = 0
    return stacks, emb, mask, memory, memory_mask


def _restated(stack, emb, mask, memory, memory_mask):
    """x = dropout(emb); per block x = x + dropout(body(norm(x))) for self-attention, cross-attention (decoder) and the
    feed-forward; dropout(final_norm(x)).  Returns that and the per-block self-attention (K, V)."""
    from modules.t5 import _attend, additive_mask
    T, dtype = emb.shape[1], emb.dtype

    def heads(t):
        return t.view(t.shape[0], t.shape[1], 2, 64).transpose(1, 2)

    def attention(att, normed, source, bias, add):
        q, k, v = heads(att.q(normed)), heads(att.k(source)), heads(att.v(source))
        out = _attend(att, q, k, v, bias, add)
        return att.o(out.transpose(1, 2).reshape(normed.shape[0], normed.shape[1], -1)), (k, v)

    keep = mask[:, None, None, :].bool()
    if stack.is_decoder:
        keep = keep & torch.ones(T, T, dtype=torch.bool).tril()[None, None]
    add = (~keep).to(dtype) * torch.finfo(dtype).min
    bias = stack.block[0].layer[0].SelfAttention.compute_bias(T, T)
    x = stack.dropout(emb)
    kvs = []
    for blk in stack.block:
        layer = blk.layer[0]
        normed = layer.layer_norm(x)
        out, kv = attention(layer.SelfAttention, normed, normed, bias, add)
        kvs.append(kv)
        x = x + layer.dropout(out)
        if stack.is_decoder:
            layer = blk.layer[1]
            out, _ = attention(layer.EncDecAttention, layer.layer_norm(x), memory, None, additive_mask(memory_mask, dtype))
            x = x + layer.dropout(out)
        layer = blk.layer[-1]
        ff = layer.DenseReluDense
        x = x + layer.dropout(ff.wo(ff.dropout(torch.relu(ff.wi(layer.layer_norm(x))))))
    return stack.dropout(stack.final_layer_norm(x)), kvs


def _forward(stack, emb, mask, memory, memory_mask, **kw):
    if stack.is_decoder:
        return stack(emb, attention_mask=mask, encoder_hidden_states=memory, encoder_attention_mask=memory_mask, **kw)
    return stack(emb, attention_mask=mask, **kw)


@pytest.mark.parametrize("decoder", [False, True])
def test_train_mode_forward_is_the_restatement_under_a_seed(decoder):
    stacks, *inputs = _setup()
    stack = stacks[decoder].train()
    with torch.no_grad():
        torch.manual_seed(SEED)
        want, want_kv = _restated(stack, *inputs)
        torch.manual_seed(SEED)
        got, got_kv = _forward(stack, *inputs, use_cache=True)
        torch.manual_seed(SEED)
        plain = _forward(stack, *inputs)
        torch.manual_seed(SEED + 1)
        other = _forward(stack, *inputs)
    assert bool(torch.isfinite(want).all()) and bool((want == 0).any())         # the last dropout was active
    assert torch.equal(got, want) and torch.equal(plain, want)
    assert len(got_kv) == len(want_kv) == 2
    for (k, v), (wk, wv) in zip(got_kv, want_kv):
        assert k.shape == (3, 2, 5, 64) and torch.equal(k, wk) and torch.equal(v, wv)
    assert not torch.equal(other, want)


@pytest.mark.parametrize("decoder", [False, True])
def test_gradients_are_the_restatement_s_under_a_seed(decoder):
    stacks, *inputs = _setup()
    stack = stacks[decoder].train()
    grads = []
    for run in (_restated, _forward):
        stack.zero_grad(set_to_none=True)
        torch.manual_seed(SEED)
        out = run(stack, *inputs)
        (out[0] if run is _restated else out).square().sum().backward()
        grads.append({n: p.grad.clone() for n, p in stack.named_parameters() if p.grad is not None})
    stack.zero_grad(set_to_none=True)
    assert sorted(grads[0]) == sorted(grads[1]) and len(grads[0]) > 15
    for n in grads[0]:
        assert torch.equal(grads[0][n], grads[1][n]), n


def test_incremental_decoder_agrees_with_the_full_length_call():
    """One position at a time with past_key_values against all five at once, in eval mode: the operators against
    themselves in fp32 at T = 5, so only rounding separates them.  Measured: max |a - b| / max |b| = 2.8e-07 for the
    hidden states, 3.1e-07 for the cached K / V (the bound is 1e-5).  A wrong mask or bias offset moves a softmax
    weight: an error of the order of the values themselves."""
    stacks, emb, mask, memory, memory_mask = _setup()
    stack = stacks[True].eval()
    with torch.no_grad():
        full, full_kv = _forward(stack, emb, mask, memory, memory_mask, use_cache=True)
        want, _ = _restated(stack, emb, mask, memory, memory_mask)
        assert torch.equal(full, want)                                           # eval mode: every dropout is off
        past, steps = None, []
        for t in range(emb.shape[1]):
            out, past = _forward(stack, emb[:, t:t + 1], mask[:, :t + 1], memory, memory_mask, past_key_values=past,
                                 use_cache=True)
            steps.append(out)
    got = torch.cat(steps, dim=1)
    err = float((got - full).abs().max() / full.abs().max())
    err_kv = max(float((a - b).abs().max() / b.abs().max()) for kv, fkv in zip(past, full_kv) for a, b in zip(kv, fkv))
    print(f"incremental vs full: hidden {err:.3e}, K/V {err_kv:.3e}")
    assert got.shape == full.shape and err <= 1e-5 and err_kv <= 1e-5
