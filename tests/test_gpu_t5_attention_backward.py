"""The trainable fused T5 attention on the GPU: ops.t5_attention_fwd_train / ops.t5_attention_bwd (csrc/t5_attention.hip)
and autograd.T5AttentionFunction against `_attend`'s operator sequence in fp64 under torch autograd, and the retrieval
model with attention_impl = "hip_train" against the reference's recorded values, "hip" and itself.

Gate: e = max|x - x64| / max|x64| per tensor, for the kernel and for the same operator sequence in fp32 on the same
inputs.  e_kernel <= 4 e_torch for `out` (the forward test's gate); e_kernel <= 8 e_torch for dq, dk, dv and the bias
table's gradient (they pass through the recomputed P and through D: two more fp32 roundings than the operators' saved
weights have).  A tensor whose fp64 reference is exactly zero must be exactly zero.  lse against fp64 logsumexp at 1e-6
relative in the same measure (retrieval_cases.lse_gate).  With dropout the reference multiplies the weights by
keep / (1 - p), keep from ops.t5_attention_dropout_keep: the contract the kernels' three recomputations of the decision
are held to.
The gate itself is retrieval_cases.gate with floor 0.  Measured ratios: profiles/retrieval_train_step.txt."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from retrieval_cases import (CASES, F32_MIN, _bias_module, _inputs, _padding, attention_train_case as _case, build_model,
                             check_forward, default_model_and_batch, fixture_batch, gate, same_bits, seed as _seed)

pytestmark = pytest.mark.gpu


def _gate(name, got, ref32, ref64, factor):
    gate(name, got, ref32, ref64, factor, floor=0.0)       # no floor here: the docstring's rule


def _encoder(T, H, p=0.0, seed=None):
    R = 5
    q, k, v, g = _inputs(R, T, R, T, H, 100 * T + H)
    att = _bias_module(H, False, T + H)
    keep = _padding(R, T, g)
    with torch.no_grad():
        table, offset = att.delta_table(T, T, 0)
    return _case(f"encoder T={T} H={H} p={p}", q, k, v, H, table=table, offset=offset, key_mask=keep, p=p, seed=seed,
                 seed_d_out=T + H, masked_row=1), v


@pytest.mark.parametrize("H", [1, 6])
@pytest.mark.parametrize("T", [1, 7, 17, 81])
def test_encoder_backward_matches_operators(T, H):
    (out, lse, dq, dk, dv, dtable, d_out), v = _encoder(T, H)
    if T == 1:   # one key: P = 1 and dS = 0 exactly
        assert same_bits(dv, d_out)
        assert not bool(dq.any()) and not bool(dk.any()) and not bool(dtable.any())


def test_encoder_backward_at_the_stated_maximum():
    from rqhip import ops
    assert ops.t5_attention_bwd_supported(torch.float32, 64, 1, 256, 256)
    assert not ops.t5_attention_bwd_supported(torch.float32, 64, 1, 257, 257)
    _encoder(256, 1)


@pytest.mark.parametrize("H", [1, 6])
@pytest.mark.parametrize("T", [2, 4])
def test_causal_backward_matches_operators(T, H):
    R = 9
    q, k, v, _ = _inputs(R, T, R, T, H, 7 * T + H)
    att = _bias_module(H, True, T)
    with torch.no_grad():
        table, offset = att.delta_table(T, T, 0)
    _case(f"causal T={T} H={H}", q, k, v, H, table=table, offset=offset, causal=True, seed_d_out=T)


@pytest.mark.parametrize("H", [1, 6])
@pytest.mark.parametrize("Tq,Tk", [(4, 81), (3, 33)])
def test_cross_backward_matches_operators(Tq, Tk, H):
    R = 6
    q, k, v, g = _inputs(R, Tq, R, Tk, H, 31 + Tq + H)
    _case(f"cross Tq={Tq} Tk={Tk} H={H}", q, k, v, H, key_mask=_padding(R, Tk, g), seed_d_out=Tk, masked_row=1)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("T", [17, 81])
def test_encoder_dropout_uses_the_contract_mask(T, p):
    from rqhip import ops
    H = 6
    (out, *_), _ = _encoder(T, H, p=p, seed=_seed(77 + T))
    R = 5
    q, k, v, g = _inputs(R, T, R, T, H, 100 * T + H)          # the inputs of _encoder again
    att = _bias_module(H, False, T + H)
    keep = _padding(R, T, g)
    with torch.no_grad():
        table, offset = att.delta_table(T, T, 0)
        other, _ = ops.t5_attention_fwd_train(q, k, v, H, bias_by_delta=table, bias_offset=offset, key_mask=keep, p=p,
                                              seed=_seed(78 + T))
    assert not torch.equal(other, out)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_cross_dropout_uses_the_contract_mask(p):
    from rqhip import ops
    R, H, Tq, Tk = 6, 6, 4, 81
    q, k, v, g = _inputs(R, Tq, R, Tk, H, 5)
    keep = _padding(R, Tk, g)
    out = _case(f"cross Tq={Tq} Tk={Tk} H={H} p={p}", q, k, v, H, key_mask=keep, p=p, seed=_seed(-3), masked_row=1)[0]
    with torch.no_grad():
        other, _ = ops.t5_attention_fwd_train(q, k, v, H, key_mask=keep, p=p, seed=_seed(4))
    assert not torch.equal(other, out)


def test_wrappers_reject_host_tensors_other_dtypes_and_beams():
    from rqhip import ops
    from rqhip._lib import RqHipError
    dev = torch.device("cuda")
    z = torch.zeros(2, 3, 64)
    with pytest.raises(RqHipError):
        ops.t5_attention_fwd_train(z, z, z, 1)
    with pytest.raises(RqHipError, match="Rk = R"):
        ops.t5_attention_fwd_train(torch.zeros(4, 1, 64, device=dev), torch.zeros(2, 8, 64, device=dev),
                                   torch.zeros(2, 8, 64, device=dev), 1)
    with pytest.raises(RqHipError, match="seed"):
        ops.t5_attention_fwd_train(z.to(dev), z.to(dev), z.to(dev), 1, p=0.1)
    with pytest.raises(RqHipError, match="float32"):
        ops.t5_attention_fwd_train(z.to(dev).half(), z.to(dev).half(), z.to(dev).half(), 1)


# ---- the autograd bridge


def test_function_equals_the_direct_calls_and_reaches_the_embedding():
    from rqhip import ops
    from rqhip.autograd import T5AttentionFunction
    R, T, H = 5, 17, 6
    q, k, v, g = _inputs(R, T, R, T, H, 3)
    att = _bias_module(H, False, 9)
    keep = _padding(R, T, g)
    w = torch.randn(R, T, H * 64, generator=g).to("cuda")
    q, k, v = (x.requires_grad_() for x in (q, k, v))
    table, offset = att.delta_table(T, T, 0)
    out = T5AttentionFunction.apply(q, k, v, table, H, offset, keep, False, 0.0, None)
    (out * w).sum().backward()
    with torch.no_grad():
        o2, lse = ops.t5_attention_fwd_train(q, k, v, H, bias_by_delta=table, bias_offset=offset, key_mask=keep)
        dq, dk, dv, dtable = ops.t5_attention_bwd(q, k, v, o2, lse, w, H, bias_by_delta=table, bias_offset=offset,
                                                  key_mask=keep)
    assert torch.equal(out, o2) and torch.equal(q.grad, dq) and torch.equal(k.grad, dk) and torch.equal(v.grad, dv)
    # the table's gradient went on through delta_table's gather to the embedding: the operators in fp64 agree
    wgrad = att.relative_attention_bias.weight.grad
    refs = []
    for dtype in (torch.float32, torch.float64):
        a2 = _bias_module(H, False, 9).to(dtype)
        bias = a2.compute_bias(T, T)
        hd = [x.detach().to(dtype).view(R, T, H, 64).transpose(1, 2) for x in (q, k, v)]
        scores = torch.matmul(hd[0], hd[1].transpose(-1, -2)) + bias + (~keep[:, None, None, :]).to(dtype) * F32_MIN
        o = torch.matmul(torch.softmax(scores, dim=-1), hd[2]).transpose(1, 2).reshape(R, T, -1)
        (o * w.to(dtype)).sum().backward()
        refs.append(a2.relative_attention_bias.weight.grad)
    _gate("embedding weight gradient", wgrad, refs[0], refs[1], 8)
    # a non-contiguous d_out (an expanded scalar, a transposed product) is accepted
    for x in (q, k, v):
        x.grad = None
    out = T5AttentionFunction.apply(q, k, v, table.detach(), H, offset, keep, False, 0.0, None)
    d_nc = w.transpose(0, 1).contiguous().transpose(0, 1)
    assert not d_nc.is_contiguous()
    out.backward(d_nc)
    assert torch.equal(q.grad, dq) and torch.equal(k.grad, dk) and torch.equal(v.grad, dv)


# ---- the model with attention_impl = "hip_train"


def _count(monkeypatch):
    import modules.t5 as t5
    calls = {"fwd": 0, "bwd": 0, "hip": 0}
    o_f, o_b, o_h = t5.ops.t5_attention_fwd_train, t5.ops.t5_attention_bwd, t5.ops.t5_attention

    def fwd(*a, **kw):
        calls["fwd"] += 1
        return o_f(*a, **kw)

    def bwd(*a, **kw):
        calls["bwd"] += 1
        return o_b(*a, **kw)

    def hip(*a, **kw):
        calls["hip"] += 1
        return o_h(*a, **kw)

    monkeypatch.setattr(t5.ops, "t5_attention_fwd_train", fwd)
    monkeypatch.setattr(t5.ops, "t5_attention_bwd", bwd)
    monkeypatch.setattr(t5.ops, "t5_attention", hip)
    return calls


@pytest.mark.parametrize("case", CASES)
def test_forward_and_gradients_match_reference_with_hip_train(case, monkeypatch):
    fx = load_golden(f"retrieval_{case}.npz")
    dev = torch.device("cuda")
    model = build_model(fx, dev).eval()
    batch = fixture_batch(fx, dev)
    model.attention_impl = "hip_train"
    calls = _count(monkeypatch)
    check_forward(fx, model, batch)
    layers = int(fx["config"][5])
    assert calls == {"fwd": 3 * layers, "bwd": 3 * layers, "hip": 0}
    with torch.no_grad():
        got = model(batch)
        assert calls == {"fwd": 3 * layers, "bwd": 3 * layers, "hip": 3 * layers}
        model.attention_impl = "hip"
        want = model(batch)
    assert same_bits(got.loss, want.loss) and same_bits(got.loss_d, want.loss_d)


def _three_steps(dev, impl):
    from modules.model import EncoderDecoderRetrievalModel
    model, batch = default_model_and_batch(dev, B=64, N=12101, d=128, seed=5)
    torch.manual_seed(5)
    model = EncoderDecoderRetrievalModel(model.codebooks, 3, 256, t5_d_model=384, t5_num_heads=6, t5_d_ff=1024,
                                         t5_num_layers=4).to(dev)
    model.attention_impl = impl
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    model.train()
    losses = []
    for _ in range(3):
        opt.zero_grad()
        out = model(batch)
        out.loss.backward()
        opt.step()
        losses.append(out.loss.item())
    assert all(torch.isfinite(p).all() for p in model.parameters())
    return losses


def test_training_steps_amazon_shape_with_hip_train(monkeypatch):
    """test_training_smoke_amazon_shape on the fused path: the kernels run under dropout, and a seeded run replays."""
    dev = torch.device("cuda")
    calls = _count(monkeypatch)
    losses = _three_steps(dev, "hip_train")
    print("losses", losses)
    assert calls == {"fwd": 3 * 3 * 4, "bwd": 3 * 3 * 4, "hip": 0}
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert _three_steps(dev, "hip_train") == losses


def test_fallbacks_under_grad_make_no_fused_call(monkeypatch):
    from modules.t5 import T5Config, T5Stack
    dev = torch.device("cuda")
    torch.manual_seed(2)
    dec = T5Stack(T5Config(16, d_model=32, num_heads=2, d_ff=32, num_layers=1, is_decoder=True)).to(dev).eval()
    enc = T5Stack(T5Config(16, d_model=32, num_heads=2, d_ff=32, num_layers=1)).to(dev).eval()
    calls = _count(monkeypatch)
    x = torch.randn(4, 3, 32, device=dev)
    memory = torch.randn(2, 5, 32, device=dev)
    long = torch.randn(1, 257, 32, device=dev)
    want = dec(x, cross_kv=dec.cross_kv(memory)), enc(long)
    dec.attention_impl = enc.attention_impl = "hip_train"
    got = dec(x, cross_kv=dec.cross_kv(memory)), enc(long)     # two beams per K/V row; a length beyond the limit
    assert calls == {"fwd": 0, "bwd": 0, "hip": 0}
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[0].requires_grad
    # ... and with one K/V per row the fused path is taken
    dec(x, cross_kv=dec.cross_kv(torch.randn(4, 5, 32, device=dev))).sum().backward()
    assert calls == {"fwd": 2, "bwd": 2, "hip": 0}
