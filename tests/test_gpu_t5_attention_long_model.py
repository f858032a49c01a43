"""The retrieval model on histories beyond the short attention kernel (modules/t5.py, `attention_long_impl = "hip"`):
d_model 32, 2 heads, 2 layers, 3 levels, separator and user token, B = 4 histories of 70 items (encoder length 281, one
row padded to a short history).  Loss and gradients against the operator model under the gate of
tests/test_gpu_t5_stack_paths.py (fp64 model, factor 4), `generate` against the cache-free operator generate as in
tests/test_gpu_t5_attention.py, which call took which kernel, the default's unchanged behaviour, and a train-mode step."""
import contextlib
import copy
import functools

import pytest
import torch

from retrieval_cases import (_cache_free_generate, compare_beams, gate, impls, loss_and_grads, same_bits, synthetic_batch,
                             to_device)

pytestmark = pytest.mark.gpu

B, L, K, ITEMS, LAYERS = 4, 3, 16, 70, 2
T_ENC = ITEMS * (L + 1) + 1


@functools.lru_cache(maxsize=None)
def _model_and_batch():
    """(fp32 model on the device, its fp64 copy on the host, the batch on both)."""
    from data.schemas import TokenizedSeqBatch
    from modules.model import EncoderDecoderRetrievalModel
    g = torch.Generator().manual_seed(5)
    torch.manual_seed(5)
    corpus = torch.randint(0, K, (300, L), generator=g)
    model = EncoderDecoderRetrievalModel(corpus, L, K, t5_d_model=32, t5_num_heads=2, t5_d_ff=64, t5_num_layers=LAYERS,
                                         should_add_sep_token=True, num_user_bins=8)
    full = synthetic_batch(corpus, B, ITEMS, g, pad="none")
    ids, mask = full.sem_ids.view(B, ITEMS, L + 1).clone(), full.seq_mask.view(B, ITEMS, L + 1).clone()
    ids[1, 6:], mask[1, 6:] = -1, False                      # row 1: a history of six items
    batch = TokenizedSeqBatch(full.user_ids, ids.view(B, -1), full.sem_ids_fut, mask.view(B, -1), None, None)
    model64 = copy.deepcopy(model).double().eval()
    return model.cuda().eval(), model64, to_device(batch, "cuda"), batch


@contextlib.contextmanager
def _setting(model, attention, long):
    with impls(model, attention=attention):
        try:
            model.attention_long_impl = long
            yield model
        finally:
            model.attention_long_impl = "torch"


@contextlib.contextmanager
def _spy(monkeypatch):
    """Every attention call of the block as (name, Tq, Tk): the six ops entry points and the operators' `_attend`."""
    import modules.t5 as t5
    calls = []

    def watch(owner, name, lengths):
        orig = getattr(owner, name)

        def spied(*a, **kw):
            calls.append((name,) + lengths(*a))
            return orig(*a, **kw)

        patch.setattr(owner, name, spied)

    with monkeypatch.context() as patch:
        for name in ("t5_attention", "t5_attention_long", "t5_attention_fwd_train", "t5_attention_long_fwd_train",
                     "t5_attention_bwd", "t5_attention_long_bwd"):
            watch(t5.ops, name, lambda q, k, *a: (q.shape[1], k.shape[1]))
        watch(t5, "_attend", lambda module, q, k, *a: (q.shape[2], k.shape[2]))
        yield calls


def _count(calls, name, Tq=None, Tk=None):
    return sum(1 for c in calls if c[0] == name and (Tq is None or c[1] == Tq) and (Tk is None or c[2] == Tk))


@functools.lru_cache(maxsize=None)
def _references():
    model, model64, batch, batch64 = _model_and_batch()
    with impls(model.eval()):
        ref32 = loss_and_grads(model, batch)
    return loss_and_grads(model64, batch64), ref32


def test_encoder_length_is_beyond_the_short_kernel():
    from modules.model import _strip_dedup_col
    model, _, batch, _ = _model_and_batch()
    with torch.no_grad():
        enc, enc_mask = model.encoder_forward_pass(attention_mask=_strip_dedup_col(batch.seq_mask.long(), L + 1, L),
                                                   input_ids=_strip_dedup_col(batch.sem_ids, L + 1, L),
                                                   user_id=batch.user_ids)
    assert enc.shape[:2] == (B, T_ENC) and T_ENC == 281
    assert int(enc_mask[1].sum()) < 40 and bool(enc_mask[0].all())


def test_loss_and_gradients_match_the_operator_model(monkeypatch):
    model, _, batch, _ = _model_and_batch()
    (loss64, grads64), (loss32, grads32) = _references()
    with _setting(model.eval(), "hip_train", "hip"), _spy(monkeypatch) as calls:
        loss, grads = loss_and_grads(model, batch)
    gate("long: loss", loss.reshape(1), loss32.reshape(1), loss64.reshape(1), 4)
    assert set(grads) == set(grads32) == set(grads64)
    for name in sorted(grads):
        gate(f"long: d {name}", grads[name], grads32[name], grads64[name], 4)
    # which call took which kernel
    assert _count(calls, "t5_attention_long_fwd_train", T_ENC, T_ENC) == LAYERS      # encoder self-attention
    assert _count(calls, "t5_attention_long_fwd_train", L + 1, T_ENC) == LAYERS      # decoder cross-attention
    assert _count(calls, "t5_attention_long_fwd_train") == 2 * LAYERS
    assert _count(calls, "t5_attention_fwd_train", L + 1, L + 1) == LAYERS           # decoder self-attention: short
    assert _count(calls, "t5_attention_fwd_train") == LAYERS
    assert _count(calls, "t5_attention_long_bwd") == 2 * LAYERS and _count(calls, "t5_attention_bwd") == LAYERS
    assert _count(calls, "_attend") == 0


def test_default_runs_the_operators_at_this_length(monkeypatch):
    model, _, batch, _ = _model_and_batch()
    (_, _), (loss32, grads32) = _references()
    with _setting(model.eval(), "hip_train", "torch"), _spy(monkeypatch) as calls:
        loss, grads = loss_and_grads(model, batch)
        with torch.no_grad():
            model.generate_next_sem_id(batch)
    assert _count(calls, "_attend") > 0 and len(calls) == _count(calls, "_attend")     # no fused attention at all
    assert same_bits(loss, loss32) and all(same_bits(grads[n], grads32[n]) for n in grads32)


def test_generate_matches_the_operator_generate(monkeypatch):
    import modules.model as mm
    model, _, batch, _ = _model_and_batch()
    k = model.top_k_for_generation
    drawn = []
    orig = mm._exponential_like

    def record(p):
        q = orig(p)
        drawn.append(q.clone())
        return q

    monkeypatch.setattr(mm, "_exponential_like", record)
    with _setting(model.eval(), "hip", "hip"), _spy(monkeypatch) as calls:
        torch.manual_seed(7)
        out = model.generate_next_sem_id(batch)
    monkeypatch.setattr(mm, "_exponential_like", orig)
    assert out.sem_ids.shape == (B, k, L) and out.log_probas.shape == (B, k)
    # encoder: one long launch per block; per step and block one cached self-attention launch of the short kernel and ONE
    # long cross-attention launch with the beams in K/V groups
    assert _count(calls, "t5_attention_long", T_ENC, T_ENC) == LAYERS
    assert _count(calls, "t5_attention_long", 1, T_ENC) == LAYERS * L
    assert _count(calls, "t5_attention_long") == LAYERS + LAYERS * L
    assert _count(calls, "t5_attention") == LAYERS * L and _count(calls, "_attend") == 0
    with impls(model.eval()):
        r_ids, r_lp, amb = _cache_free_generate(model, batch, drawn)
    n_amb = compare_beams(out.sem_ids, out.log_probas, None, r_ids, r_lp, None, amb, 1e-5, 1e-5)
    print(f"long generate: {n_amb}/{B} users inside the gap, {int(torch.isfinite(r_lp).sum())} finite beams")
    assert n_amb <= B // 2 and torch.isfinite(out.log_probas).any()
    with _setting(model.eval(), "hip", "hip"):
        torch.manual_seed(7)
        again = model.generate_next_sem_id(batch)
    assert torch.equal(again.sem_ids, out.sem_ids) and same_bits(again.log_probas, out.log_probas)


def test_train_mode_step_with_dropout_repeats_bit_for_bit(monkeypatch):
    model, _, batch, _ = _model_and_batch()
    assert model.t5_decoder.config.dropout_rate == 0.1
    try:
        with _setting(model.train(), "hip_train", "hip"), _spy(monkeypatch) as calls:
            loss, grads = loss_and_grads(model, batch, seed=3)
            n_first = len(calls)
            loss2, grads2 = loss_and_grads(model, batch, seed=3)
            loss3, _ = loss_and_grads(model, batch, seed=4)
    finally:
        model.eval()
    assert _count(calls, "t5_attention_long_fwd_train") == 3 * (2 * LAYERS) and _count(calls, "_attend") == 0
    assert len(calls) == 3 * n_first
    assert torch.isfinite(loss) and all(torch.isfinite(g).all() for g in grads.values())
    assert same_bits(loss.reshape(1), loss2.reshape(1)) and set(grads) == set(grads2)
    assert all(same_bits(grads[n], grads2[n]) for n in grads)
    assert not torch.equal(loss, loss3)                       # another seed, other masks
