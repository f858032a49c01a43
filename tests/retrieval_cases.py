"""What the retrieval-model tests share: the accuracy gate, the bit comparisons, the synthetic batch, the small, tiny,
default and fixture models, the switch between kernel implementations, the operator restatements of the beam step
and of the attention inputs, the fused attention's operator references, gates and training case, and the log of a
train-mode step's dropout masks with its replay on the operators.

Test infrastructure like tests/parity_gate.py: imported by the tests and by tools/bench_retrieval_train.py and
tools/bench_generate.py (which put tests/ on sys.path); the product package never imports it, and it imports the product
only inside its functions."""
import collections
import contextlib
import copy
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

# ---- the gate: e = max|a - a64| / max|a64| per tensor, e_kernel <= max(factor * e_torch, floor)

FLOOR = 2.0 ** -22      # two fp32 ulps of the largest element, for the cases in which the operators happen to be exact


def err(a, a64):
    return float((a.to(a64.device).double() - a64).abs().max() / a64.abs().max())


def gate(name, got, ref32, ref64, factor, floor=FLOOR):
    """Prints and asserts the gate of `got` (the kernel) and `ref32` (the operators in fp32 on the same inputs) against
    `ref64`.  A tensor whose fp64 reference is exactly zero must be exactly zero."""
    assert torch.isfinite(got).all(), name
    if not bool(ref64.any()):
        print(f"{name}: the fp64 reference is exactly zero")
        assert not bool(got.any()), name
        return
    e_kernel, e_torch = err(got, ref64), err(ref32, ref64)
    ratio = e_kernel / e_torch if e_torch > 0 else (0.0 if e_kernel == 0 else float("inf"))
    print(f"{name}: e_kernel {e_kernel:.3e} e_torch {e_torch:.3e} ratio {ratio:.2f}")
    assert e_kernel <= max(factor * e_torch, floor), name


# ---- small helpers


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def seed(value):
    return torch.tensor([value], dtype=torch.int64, device="cuda")


def loss_and_grads(model, batch, seed=None):
    model.zero_grad(set_to_none=True)
    if seed is not None:
        torch.manual_seed(seed)
    loss = model(batch).loss
    loss.backward()
    return loss.detach(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


@contextlib.contextmanager
def impls(model, *, attention="torch", norm="torch", ffn="torch", head="torch"):
    """The four implementation choices on `model` and both of its stacks inside the block; after it, also when it
    raised, all four are "torch" again, the model is in the mode (train / eval) it came in and has no gradients."""
    def put(*choice):
        model.attention_impl, model.norm_impl, model.ffn_impl, model.head_impl = choice
        model._push_attention_impl()

    training = model.training
    put(attention, norm, ffn, head)
    try:
        yield model
    finally:
        put("torch", "torch", "torch", "torch")
        model.train(training)
        model.zero_grad(set_to_none=True)


# ---- the batch: histories with the dedup column, padded tails, future ids, user ids, drawn in that order


def synthetic_batch(corpus, B, items, generator, *, pad="none", user_ids=True):
    """A host TokenizedSeqBatch of B users with `items` corpus rows each.  pad: "none", "row1" (the last item of user 1)
    or "b_mod_items" (the last b % items items of user b); a padded id is -1 and its mask False.  user_ids False: zeros,
    and no draw."""
    from data.schemas import TokenizedSeqBatch
    N, L = corpus.shape
    hist = torch.cat([corpus[torch.randint(0, N, (B, items), generator=generator)],
                      torch.zeros(B, items, 1, dtype=torch.long)], dim=-1)
    mask = torch.ones(B, items, L + 1, dtype=torch.bool)
    tails = {"none": {}, "row1": {1: 1}, "b_mod_items": {b: b % items for b in range(B) if b % items}}[pad]
    for b, n in tails.items():
        hist[b, items - n:] = -1
        mask[b, items - n:] = False
    fut = torch.cat([corpus[torch.randint(0, N, (B,), generator=generator)], torch.zeros(B, 1, dtype=torch.long)], dim=-1)
    users = torch.randint(0, 100, (B, 1), generator=generator) if user_ids else torch.zeros(B, 1, dtype=torch.long)
    return TokenizedSeqBatch(users, hist.reshape(B, -1), fut, mask.reshape(B, -1), None, None)


def to_device(batch, dev):
    return type(batch)(*[None if t is None else t.to(dev) for t in batch])


# ---- models

LAYERS = 2


@functools.lru_cache(maxsize=None)
def small_model(seed, d_ff, perturb_norms, device="cuda", items=2):
    """(fp32 model on the device, its fp64 copy on the host, the batch on both) -- built once: d_model 64, 2 heads, 2
    layers, K = 16, L = 3, batch 3 with one padded row; decoder T = 4, encoder T = 4 * items (three ids and the separator
    per item of the history)."""
    from modules.model import EncoderDecoderRetrievalModel
    B, L, K, N = 3, 3, 16, 200
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    corpus = torch.randint(0, K, (N, L), generator=g)
    model = EncoderDecoderRetrievalModel(corpus, L, K, t5_d_model=64, t5_num_heads=2, t5_d_ff=d_ff, t5_num_layers=LAYERS)
    if perturb_norms:                              # norm weights away from 1, some negative: their gradients matter
        with torch.no_grad():
            for name, p in model.named_parameters():
                if name.endswith("layer_norm.weight"):
                    p.copy_(1 + 0.5 * torch.randn(p.shape, generator=g))
    batch = synthetic_batch(corpus, B, items, g, pad="row1")
    model64 = copy.deepcopy(model).double().eval()
    return model.to(device).eval(), model64, to_device(batch, device), batch


@functools.lru_cache(maxsize=None)
def reference(seed, d_ff, perturb_norms):
    """loss_and_grads of small_model's fp64 copy."""
    _, model64, _, batch = small_model(seed, d_ff, perturb_norms)
    return loss_and_grads(model64, batch)


def tiny_model(d_model=8, d_ff=8):
    from modules.model import EncoderDecoderRetrievalModel
    torch.manual_seed(0)
    return EncoderDecoderRetrievalModel(torch.zeros(4, 3, dtype=torch.long), 3, 16, t5_d_model=d_model, t5_num_heads=2,
                                        t5_d_ff=d_ff, t5_num_layers=1)


def tiny_batch():
    from data.schemas import TokenizedSeqBatch
    g = torch.Generator().manual_seed(1)
    return TokenizedSeqBatch(torch.zeros(2, 1, dtype=torch.long), torch.randint(0, 16, (2, 8), generator=g),
                             torch.randint(0, 16, (2, 4), generator=g), torch.ones(2, 8, dtype=torch.bool), None, None)


def _corpus(K, L, N, g, dev):
    base = torch.randint(0, K, (N, L), generator=g)
    # shared prefixes: a third of the rows copy another row's first L - 1 ids
    m = N // 3
    base[:m, : L - 1] = base[torch.randint(m, N, (m,), generator=g), : L - 1]
    return base.to(dev)


def default_model_and_batch(dev, B=64, N=20000, items=20, d=128, L=3, K=256, seed=0):
    from modules.model import EncoderDecoderRetrievalModel
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    corpus = _corpus(K, L, N, g, "cpu")
    model = EncoderDecoderRetrievalModel(corpus, L, K, t5_d_model=d).to(dev).eval()
    with torch.no_grad():
        for lin in model.decoder_mlp:
            lin.weight.mul_(8.0)
    return model, to_device(synthetic_batch(corpus, B, items, g, pad="b_mod_items"), dev)


# ---- the reference's recorded runs (tests/golden/retrieval_*.npz, tools/gen_retrieval_golden.py)

CASES = ("a", "b", "c")


def build_model(fx, device="cpu"):
    """The fixture's model with its recorded weights (the unused shared / embed_tokens tables filled with zeros)."""
    from modules.model import EncoderDecoderRetrievalModel
    L, K, d, heads, d_ff, layers, sep, bins, k = (int(v) for v in fx["config"])
    corpus = torch.from_numpy(fx["corpus"])
    model = EncoderDecoderRetrievalModel(corpus, L, K, t5_d_model=d, t5_num_heads=heads, t5_d_ff=d_ff,
                                         t5_num_layers=layers, top_k_for_generation=k, should_add_sep_token=bool(sep),
                                         num_user_bins=bins or None)
    sd = {name: torch.zeros_like(v) for name, v in model.state_dict().items()}
    for name in list(sd):
        if "w." + name in fx:
            sd[name] = torch.from_numpy(fx["w." + name])
    model.load_state_dict(sd, strict=True)
    return model.to(device)


def fixture_batch(fx, device="cpu"):
    from data.schemas import TokenizedSeqBatch
    return TokenizedSeqBatch(*[torch.from_numpy(fx["batch." + f]).to(device) for f in TokenizedSeqBatch._fields])


def check_forward(fx, model, batch):
    model.eval()
    model.zero_grad()
    out = model(batch)
    out.loss.backward()
    assert out.logits is None
    np.testing.assert_allclose(out.loss.item(), float(fx["loss"]), rtol=1e-5)
    np.testing.assert_allclose(out.loss_d.cpu().numpy(), fx["loss_d"], rtol=1e-5)
    seen = 0
    for name, p in model.named_parameters():
        if "g." + name in fx:
            want = fx["g." + name]
            scale = max(float(np.abs(want).max()), 1e-6)
            got = p.grad.detach().cpu().numpy()
            np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4 * scale, err_msg=name)
            seen += 1
        else:  # no gradient in the reference: the unused tables
            assert p.grad is None or not p.grad.any(), name
    assert seen > 10


# ---- the beam step as the reference's operators, and what compares two sets of beams

GAP = 1e-5


def _close(a, b):
    """|a - b| within GAP relative (two equal values, -inf included, are close)."""
    both_inf = torch.isinf(a) & torch.isinf(b) & (a == b)
    finite = torch.isfinite(a) & torch.isfinite(b)
    return both_inf | (finite & ((a - b).abs() <= GAP * torch.maximum(a.abs(), b.abs())))


def ref_beam_step(logits, noise, parent_scores, parent_ids, index, corpus, n, k):
    """The reference's step as torch operators: softmax, topk(p / q) (multinomial without replacement), gather, log,
    prefix lookup, masked_fill, stable descending sort, gathers.  Also returns, per user, whether an order the kernel
    may legitimately resolve differently decides the outcome (a gap within 1e-5 relative)."""
    from rqhip import ops
    rows, K = logits.shape
    beams_in = 1 if parent_ids is None else parent_ids.shape[1]
    h = 0 if parent_ids is None else parent_ids.shape[2]
    B = rows // beams_in
    p = F.softmax(logits, dim=-1)
    keys = p / noise
    kv, order = torch.sort(keys, dim=-1, descending=True, stable=True)
    samples = order[:, :n]
    lp = torch.log(torch.gather(p, 1, samples))
    if h:
        prev = parent_ids.repeat_interleave(n, dim=1)                       # [B, beams_in * n, h]
        prefix = torch.cat([prev, samples.reshape(B, beams_in * n, 1)], dim=-1)
        scores = lp.reshape(B, beams_in * n) + parent_scores.repeat_interleave(n, dim=1)
    else:
        prefix = samples.reshape(B, n, 1)
        scores = lp.reshape(B, n)
    valid = ops.prefix_lookup(index, corpus, prefix.reshape(-1, h + 1)).reshape(B, -1)
    scores = scores.masked_fill(~valid, float("-inf"))
    sv, idx = torch.sort(scores, dim=-1, descending=True, stable=True)
    top = idx[:, :k]
    ids = torch.gather(prefix, 1, top.unsqueeze(-1).expand(-1, -1, h + 1))
    parent = top // n + torch.arange(B, device=logits.device).unsqueeze(1) * beams_in
    # ambiguity: the n-th vs the (n+1)-th nonzero key of a row (which codes are sampled; the order inside the n only
    # numbers the candidates, which matters between equal scores alone), neighbouring finite scores among the first
    # k + 1 of a user (which candidates are kept, and their order)
    if n < K:
        key_tie = (_close(kv[:, n - 1], kv[:, n]) & (kv[:, n - 1] > 0)).reshape(B, beams_in).any(dim=1)
    else:
        key_tie = torch.zeros(B, dtype=torch.bool, device=logits.device)
    ss = sv[:, : min(k + 1, sv.shape[1])]
    score_tie = (_close(ss[:, :-1], ss[:, 1:]) & torch.isfinite(ss[:, :-1])).any(dim=1)
    return ids, sv[:, :k], parent, key_tie | score_tie


def compare_beams(ids, scores, parent, r_ids, r_scores, r_parent, ambiguous, score_atol, score_rtol=0.0):
    """Equal ids / parents at every kept beam with a finite reference score, of every user whose outcome no
    near-tie decides; scores within score_atol or both -inf everywhere.  Returns the number of ambiguous users."""
    fin = torch.isfinite(r_scores)
    assert torch.equal(torch.isfinite(scores), fin), "-inf beams differ"
    np.testing.assert_allclose(scores[fin].cpu().numpy(), r_scores[fin].cpu().numpy(), rtol=score_rtol,
                               atol=score_atol)
    ok = (~ambiguous).unsqueeze(1) & fin
    assert torch.equal(ids[ok], r_ids[ok]), "ids differ"
    if parent is not None:
        assert torch.equal(parent[ok], r_parent[ok]), "parents differ"
    return int(ambiguous.sum())


class _Replay:
    """Stands in for modules.model._exponential_like: hands out given noise tensors in order."""

    def __init__(self, noise):
        self.noise = list(noise)
        self.i = 0

    def __call__(self, probas):
        q = self.noise[self.i]
        self.i += 1
        assert q.shape == probas.shape
        return q


def _cache_free_generate(model, batch, noise):
    """generate() with every step decoded in full (BOS + all ids so far, no cache) and the reference's operators."""
    from modules.model import _strip_dedup_col
    L, K, k = model.num_hierarchies, model.num_embeddings_per_hierarchy, model.top_k_for_generation
    n = min(64, K)
    ids_in = _strip_dedup_col(batch.sem_ids, L + 1, L)
    mask = _strip_dedup_col(batch.seq_mask.long(), L + 1, L)
    idx = model._prefix_index_for_codebooks()
    with torch.no_grad():
        enc, enc_mask = model.encoder_forward_pass(mask, ids_in, batch.user_ids)
        B = enc.shape[0]
        ids = scores = None
        amb_any = torch.zeros(B, dtype=torch.bool, device=enc.device)
        for h in range(L):
            if h == 0:
                hid = model.decoder_forward_pass(encoder_output=enc, attention_mask_for_encoder=enc_mask)
            else:
                hid = model.decoder_forward_pass(future_ids=ids.reshape(-1, h),
                                                 encoder_output=enc.repeat_interleave(k, dim=0),
                                                 attention_mask_for_encoder=enc_mask.repeat_interleave(k, dim=0))
            logits = model.decoder_mlp[h](hid[:, -1])
            ids, scores, _, amb = ref_beam_step(logits, noise[h], scores, ids, idx._index, idx._corpus, n, k)
            amb_any |= amb
    return ids, scores, amb_any


# ---- inputs of the fused attention's tests


def _inputs(R, Tq, Rk, Tk, H, seed):
    g = torch.Generator().manual_seed(seed)
    dev = torch.device("cuda")
    q = (torch.randn(R, Tq, H * 64, generator=g) * 1.5).to(dev)   # no 1/sqrt(d): scores reach 30 and beyond
    k = torch.randn(Rk, Tk, H * 64, generator=g).to(dev)
    v = torch.randn(Rk, Tk, H * 64, generator=g).to(dev)
    return q, k, v, g


def _bias_module(H, is_decoder, seed):
    from modules.t5 import T5Attention, T5Config
    torch.manual_seed(seed)
    att = T5Attention(T5Config(64, d_model=32, num_heads=H, is_decoder=is_decoder), has_relative_attention_bias=True)
    torch.nn.init.normal_(att.relative_attention_bias.weight)
    return att.to("cuda")


def _padding(R, T, g):
    """Keep-mask [R, T] with padded tails of every length; row 1 (if any) is fully masked."""
    keep = torch.arange(T)[None, :] < torch.randint(1, T + 1, (R, 1), generator=g)
    keep[0] = True
    if R > 1:
        keep[1] = False
    return keep.to("cuda")


# ---- the fused attention against the operators: the inference kernel's reference and gate (test_gpu_t5_attention.py's
# docstring), the training pair's reference, lse gate and case (test_gpu_t5_attention_backward.py's docstring)

_EVAL = types.SimpleNamespace(dropout=0.0, training=False)

F32_MIN = torch.finfo(torch.float32).min   # what is ADDED to a masked score, in the fp64 reference too


def attention_operators(q, k, v, H, bias, keep, dtype):
    """modules/t5.py's sequence (head transposes, _attend, transpose back) in `dtype`.  q [R, Tq, H*64], k / v
    [R, Tk, H*64], bias [1, H, Tq, Tk] or None, keep [R, 1, Tq or 1, Tk] bool or None."""
    from modules.t5 import _attend

    def heads(x):
        return x.to(dtype).view(x.shape[0], x.shape[1], H, 64).transpose(1, 2)

    mask = None if keep is None else (~keep).to(dtype) * torch.finfo(dtype).min
    bias = None if bias is None else bias.to(dtype)
    if dtype == torch.float32:
        out = _attend(_EVAL, heads(q), heads(k), heads(v), bias, mask)
    else:  # _attend's sequence with its softmax in `dtype` too (its `.float()` is the identity in fp32 only)
        scores = torch.matmul(heads(q), heads(k).transpose(-1, -2))
        if bias is not None:
            scores = scores + bias
        if mask is not None:
            scores = scores + mask
        out = torch.matmul(torch.softmax(scores, dim=-1), heads(v))
    return out.transpose(1, 2).reshape(q.shape[0], q.shape[1], -1)


def attention_gate(name, out, q, k, v, H, bias, keep):
    """Prints and asserts the inference kernel's gate (e_kernel <= 4 e_torch, equality at Tk = 1); k / v already expanded
    to one K/V per query row.  Returns the largest |score|."""
    out64 = attention_operators(q, k, v, H, bias, keep, torch.float64)
    out32 = attention_operators(q, k, v, H, bias, keep, torch.float32)
    e_kernel, e_torch = err(out, out64), err(out32, out64)
    smax = float(torch.einsum("rihd,rjhd->rhij", q.double().view(*q.shape[:2], H, 64),
                              k.double().view(*k.shape[:2], H, 64)).abs().max())
    ratio = e_kernel / e_torch if e_torch > 0 else (0.0 if e_kernel == 0 else float("inf"))
    print(f"{name}: e_kernel {e_kernel:.3e} e_torch {e_torch:.3e} ratio {ratio:.2f} max|score| {smax:.1f}")
    assert torch.isfinite(out).all()
    if k.shape[1] == 1:
        assert e_kernel == e_torch
    else:
        assert e_kernel <= 4 * e_torch
    return smax


def attention_train_operators(q, k, v, H, table, offset, keep, drop, p, d_out, dtype):
    """`_attend`'s sequence with its head transposes in `dtype` under autograd -> (out, lse, dq, dk, dv, dtable).
    table [n_delta, H] or None (bias[h, i, j] = table[j - i + offset, h]); keep [R, 1, Tq or 1, Tk] bool or None;
    drop [R, H, Tq, Tk] bool or None."""
    Tq, Tk = q.shape[1], k.shape[1]
    q, k, v = (x.detach().to(dtype).requires_grad_() for x in (q, k, v))
    leaves = [q, k, v]

    def heads(x):
        return x.view(x.shape[0], x.shape[1], H, 64).transpose(1, 2)

    scores = torch.matmul(heads(q), heads(k).transpose(-1, -2))
    if table is not None:
        table = table.detach().to(dtype).requires_grad_()
        leaves.append(table)
        i = torch.arange(Tq, device=q.device)[:, None]
        j = torch.arange(Tk, device=q.device)[None, :]
        scores = scores + table[(j - i) + offset].permute(2, 0, 1).unsqueeze(0)
    if keep is not None:
        scores = scores + (~keep).to(dtype) * F32_MIN
    lse = torch.logsumexp(scores.detach(), dim=-1)
    weights = torch.softmax(scores, dim=-1)
    if drop is not None:
        weights = weights * (drop.to(dtype) / (1 - p))
    out = torch.matmul(weights, heads(v)).transpose(1, 2).reshape(q.shape[0], Tq, -1)
    grads = torch.autograd.grad(out, leaves, d_out.to(dtype))
    return (out.detach(), lse) + tuple(grads) + ((None,) if table is None else ())


def lse_gate(name, lse, lse64):
    """max|lse - lse64| / max|lse64| <= 1e-6, the error measure of the module docstring: a score is a 64-term fp32 dot
    product whose error is relative to its terms, not to a sum that may cancel to nothing, so an element-wise relative
    bound is not one fp32 can meet.  Rows with every key masked (|lse| = 3.4e38) are measured apart from the others, so
    that their size does not hide the others' error."""
    big = lse64.abs() > 1e30
    for what, sel in (("masked rows", big), ("other rows", ~big)):
        if bool(sel.any()):
            e = err(lse[sel], lse64[sel])
            print(f"{name} lse, {what}: e_kernel {e:.3e}")
            assert e <= 1e-6, name


def attention_train_case(name, q, k, v, H, *, table=None, offset=0, key_mask=None, causal=False, p=0.0, seed=None,
                         seed_d_out=0, masked_row=None):
    """One shape through fwd_train and bwd: p = 0 bits of the inference kernel, every gate (no floor: the rule of
    test_gpu_t5_attention_backward.py's docstring), the fully masked row on its own, and a second run with identical
    bits.  Returns the kernel's tensors."""
    from rqhip import ops
    R, Tq, Tk = q.shape[0], q.shape[1], k.shape[1]
    dev = q.device
    d_out = torch.randn(R, Tq, H * 64, generator=torch.Generator().manual_seed(1000 + seed_d_out)).to(dev)
    kw = dict(bias_by_delta=table, bias_offset=offset, key_mask=key_mask, causal=causal)

    def run():
        out, lse = ops.t5_attention_fwd_train(q, k, v, H, p=p, seed=seed, **kw)
        return (out, lse) + tuple(ops.t5_attention_bwd(q, k, v, out, lse, d_out, H, p=p, seed=seed, **kw))

    with torch.no_grad():
        got = run()
        if p == 0:
            assert same_bits(got[0], ops.t5_attention(q, k, v, H, **kw))
    keep = None if key_mask is None else key_mask[:, None, None, :]
    if causal:
        tri = torch.ones(Tq, Tk, dtype=torch.bool, device=dev).tril()[None, None]
        keep = tri if keep is None else keep & tri
    drop = ops.t5_attention_dropout_keep(seed, R, H, Tq, Tk, p) if p > 0 else None
    ref64 = attention_train_operators(q, k, v, H, table, offset, keep, drop, p, d_out, torch.float64)
    ref32 = attention_train_operators(q, k, v, H, table, offset, keep, drop, p, d_out, torch.float32)
    lse_gate(name, got[1], ref64[1])
    gate(f"{name} out", got[0], ref32[0], ref64[0], 4, floor=0.0)
    for n, x, x32, x64 in zip(("dq", "dk", "dv", "dtable"), got[2:], ref32[2:], ref64[2:]):
        assert (x is None) == (x64 is None)
        if x is not None:
            gate(f"{name} {n}", x, x32, x64, 8, floor=0.0)
    if masked_row is not None and Tk > 1:     # every key masked: uniform P, dS != 0, no special case anywhere
        assert not bool(key_mask[masked_row].any()) and bool(ref64[2][masked_row].any())
        for n, x, x32, x64 in zip(("dq", "dk", "dv"), got[2:5], ref32[2:5], ref64[2:5]):
            gate(f"{name} {n} of the fully masked row", x[masked_row], x32[masked_row], x64[masked_row], 8, floor=0.0)
    with torch.no_grad():
        again = run()
    for x, y in zip(got, again):
        assert (x is None and y is None) or same_bits(x, y)
    return got + (d_out,)


# ---- train-mode steps: the dropout masks a step used, logged site by site, and their replay on the operators
#
# A site is one dropout of a forward.  Their order is the same on every path (modules/t5.py): per stack the input
# embeddings, then per block the self-attention weights, the sub-layer output, (decoder) the cross-attention weights,
# the sub-layer output, the feed-forward's inner activation, the sub-layer output -- the last of these is the final p_in
# -- and the final norm's output.


class SiteMismatch(AssertionError):
    """A replay met a dropout the log does not hold, holds with another shape or rate, or left sites of the log over."""


Site = collections.namedtuple("Site", "kind p keep seed")          # kind: attention, glue_in, glue_out, ffn, operator
Call = collections.namedtuple("Call", "op direction seed p shapes")  # one spied ops call; seed: its value or None


class MaskLog:
    """The keep masks of one forward in chronological order (`sites`), and the fused ops calls that were spied while
    they were recorded (`calls`, backward calls included)."""

    def __init__(self, sites=(), calls=()):
        self.sites, self.calls = list(sites), list(calls)

    def __len__(self):
        return len(self.sites)

    def swapped(self, i, keep):
        """A copy in which site i has the mask `keep`."""
        assert keep.shape == self.sites[i].keep.shape and keep.dtype == torch.bool
        sites = list(self.sites)
        sites[i] = sites[i]._replace(keep=keep)
        return MaskLog(sites, self.calls)

    def without(self, i):
        """A copy that lacks site i."""
        return MaskLog(self.sites[:i] + self.sites[i + 1:], self.calls)

    def fused(self, direction):
        return [c for c in self.calls if c.direction == direction]


def _dropped(x, keep, p):
    return x * keep.to(x.device) * (1.0 / (1.0 - p))


def _seed_value(seed):
    return None if seed is None else int(seed)


@contextlib.contextmanager
def _patched(owner, **replacements):
    saved = {name: getattr(owner, name) for name in replacements}
    for name, fn in replacements.items():
        setattr(owner, name, fn)
    try:
        yield
    finally:
        for name, fn in saved.items():
            setattr(owner, name, fn)


@contextlib.contextmanager
def recording(draw_seed=0):
    """Inside the block every dropout of a model step is logged -> the MaskLog.  Fused sites: the three ops entry
    points the Functions of rqhip/autograd.py call are spied, with their _bwd counterparts, and a forward call's masks
    are rebuilt from its own seed, p and shapes by the kernels' published decision (ops.t5_attention_dropout_keep, in
    the conventions of test_gpu_t5_add_norm.py:_masks and test_gpu_t5_ffn.py:_keep).  Operator sites:
    torch.nn.functional.dropout is a stand-in that draws an explicit Bernoulli mask from a generator seeded with
    `draw_seed` and applies x * keep * (1 / (1 - p))."""
    from rqhip import ops
    log = MaskLog()
    g = torch.Generator().manual_seed(draw_seed)
    o = {n: getattr(ops, n) for n in ("t5_attention_fwd_train", "t5_attention_bwd", "t5_add_norm_fwd", "t5_add_norm_bwd",
                                      "t5_ffn_fwd", "t5_ffn_bwd")}

    def site(kind, p, keep, seed, shape):
        log.sites.append(Site(kind, float(p), keep.view(shape), _seed_value(seed)))

    def attention_fwd(q, k, v, n_heads, **kw):
        p, seed = kw.get("p", 0.0), kw.get("seed")
        log.calls.append(Call("attention", "fwd", _seed_value(seed), (p,), (q.shape, k.shape, v.shape)))
        if p > 0:
            R, Tq, Tk = q.shape[0], q.shape[1], k.shape[1]
            site("attention", p, ops.t5_attention_dropout_keep(seed, R, n_heads, Tq, Tk, p), seed, (R, n_heads, Tq, Tk))
        return o["t5_attention_fwd_train"](q, k, v, n_heads, **kw)

    def attention_bwd(q, k, v, out, lse, d_out, n_heads, **kw):
        log.calls.append(Call("attention", "bwd", _seed_value(kw.get("seed")), (kw.get("p", 0.0),),
                              (q.shape, k.shape, v.shape)))
        return o["t5_attention_bwd"](q, k, v, out, lse, d_out, n_heads, **kw)

    def add_norm_fwd(x, y, w, eps, p_in=0.0, p_out=0.0, seed=None):
        from test_gpu_t5_add_norm import _masks
        log.calls.append(Call("glue", "fwd", _seed_value(seed), (p_in, p_out), (y.shape,)))
        d = y.shape[-1]
        keep_in, keep_out = _masks(seed, y.numel() // d, d, p_in, p_out) if p_in > 0 or p_out > 0 else (None, None)
        if keep_in is not None:
            site("glue_in", p_in, keep_in, seed, y.shape)
        if keep_out is not None:
            site("glue_out", p_out, keep_out, seed, y.shape)
        return o["t5_add_norm_fwd"](x, y, w, eps, p_in, p_out, seed)

    def add_norm_bwd(x_new, rstd, w, d_n, d_xnew, p_in=0.0, p_out=0.0, seed=None, **kw):
        log.calls.append(Call("glue", "bwd", _seed_value(seed), (p_in, p_out), (x_new.shape,)))
        return o["t5_add_norm_bwd"](x_new, rstd, w, d_n, d_xnew, p_in, p_out, seed, **kw)

    def ffn_fwd(x, wi, wo, p=0.0, seed=None, **kw):
        from test_gpu_t5_ffn import _keep
        F_ = wi.shape[0]
        log.calls.append(Call("ffn", "fwd", _seed_value(seed), (p,), (x.shape, x.shape[:-1] + (F_,))))
        keep = _keep(seed, x.numel() // x.shape[-1], F_, p)
        if keep is not None:
            site("ffn", p, keep, seed, x.shape[:-1] + (F_,))
        return o["t5_ffn_fwd"](x, wi, wo, p, seed, **kw)

    def ffn_bwd(x, wi, wo, h, d_y, p=0.0, seed=None, **kw):
        log.calls.append(Call("ffn", "bwd", _seed_value(seed), (p,), (x.shape, h.shape)))
        return o["t5_ffn_bwd"](x, wi, wo, h, d_y, p, seed, **kw)

    def drawn(input, p=0.5, training=True, inplace=False):
        if not training or p == 0:
            return input
        keep = torch.rand(input.shape, generator=g) >= p
        log.sites.append(Site("operator", float(p), keep.to(input.device), None))
        return _dropped(input, keep, p)

    with _patched(ops, t5_attention_fwd_train=attention_fwd, t5_attention_bwd=attention_bwd, t5_add_norm_fwd=add_norm_fwd,
                  t5_add_norm_bwd=add_norm_bwd, t5_ffn_fwd=ffn_fwd, t5_ffn_bwd=ffn_bwd), _patched(F, dropout=drawn):
        yield log


@contextlib.contextmanager
def replaying(log):
    """Inside the block torch.nn.functional.dropout hands out the masks of `log` in order.  A dropout the log does not
    hold, or holds with another shape or rate, raises SiteMismatch with the site's index and shape; so does a block
    that ends (without another error) with sites left over."""
    at = [0]

    def popped(input, p=0.5, training=True, inplace=False):
        if not training or p == 0:
            return input
        i, shape = at[0], tuple(input.shape)
        if i >= len(log.sites):
            raise SiteMismatch(f"site {i}: the model drops a tensor of shape {shape} at p = {p}, the log ends after "
                               f"{len(log.sites)} sites")
        s = log.sites[i]
        if tuple(s.keep.shape) != shape or s.p != float(p):
            raise SiteMismatch(f"site {i}: the model drops a tensor of shape {shape} at p = {p}, the log holds the "
                               f"{s.kind} mask of shape {tuple(s.keep.shape)} at p = {s.p}")
        at[0] += 1
        return _dropped(input, s.keep, p)

    with _patched(F, dropout=popped):
        yield
    if at[0] != len(log.sites):
        s = log.sites[at[0]]
        raise SiteMismatch(f"site {at[0]}: the log's {s.kind} mask of shape {tuple(s.keep.shape)} at p = {s.p} and "
                           f"{len(log.sites) - at[0] - 1} sites behind it were never asked for")


@contextlib.contextmanager
def setting(model, *, attention="torch", norm="torch", ffn="torch", head="torch", embed="torch", proj="torch"):
    """`impls` with the model's two other choices, embed_impl and proj_impl; after the block those are "torch" too."""
    with impls(model, attention=attention, norm=norm, ffn=ffn, head=head):
        try:
            model.embed_impl, model.proj_impl = embed, proj
            model._push_attention_impl()
            yield model
        finally:
            model.embed_impl = model.proj_impl = "torch"


def _train_step(model, batch, seed):
    training = model.training
    try:
        return loss_and_grads(model.train(), batch, seed=seed)
    finally:
        model.train(training)
        model.zero_grad(set_to_none=True)


def record_step(model, batch, seed=None, draw_seed=0):
    """One train-mode forward and backward of `model` as it is set up -> (loss, gradients, MaskLog).  `seed`:
    torch.manual_seed before the step (the fused sites' seeds); `draw_seed`: the generator of the operator sites.  The
    model comes back in the mode it had."""
    with recording(draw_seed) as log:
        loss, grads = _train_step(model, batch, seed)
    return loss, grads, log


def replay_step(model, batch, log):
    """record_step's loss and gradients of `model`, every mask taken from `log` (replaying)."""
    with replaying(log):
        return _train_step(model, batch, None)
