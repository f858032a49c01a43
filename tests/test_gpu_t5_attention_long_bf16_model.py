"""The retrieval model with `attention_arith = "bf16"` (modules/t5.py) on the tiny model and batch of
tests/test_gpu_t5_attention_long_model.py (encoder length 281, one short row): which calls carry the arithmetic, the
default's unchanged calls, the eval-mode loss and a train-mode step against the fp32 arm of the same setting, and
`generate`.

The thresholds.  The relative loss difference stays below the project's sanity cap 2^-6 (profiles/t5_bf16_error.txt, 3).
The tight ones -- the loss, and per parameter max|g_bf16 - g_fp32| / max|g_fp32| -- are 4 times the largest value of
eight seeds measured against the fp32 arm (`measure`; the table is in profiles/t5_attention_long_bf16.txt): eight seeds
are a small sample."""
import contextlib

import pytest
import torch

from retrieval_cases import impls, loss_and_grads, same_bits
from test_gpu_t5_attention_long_model import LAYERS, L, T_ENC, B, _model_and_batch

pytestmark = pytest.mark.gpu

SANITY_CAP = 2.0 ** -6
ABSENT = "<no keyword>"
LONG_OPS = ("t5_attention_long", "t5_attention_long_fwd_train", "t5_attention_long_bwd")
SHORT_OPS = ("t5_attention", "t5_attention_fwd_train", "t5_attention_bwd")
SEEDS = (3, 4, 5, 6, 7, 8, 9, 10)

# 4 x the largest value of `measure(SEEDS)` (profiles/t5_attention_long_bf16.txt): relative loss difference in eval and
# train mode, and max|dg| / max|g_fp32| of a train-mode step by parameter
MEASURED_LOSS_EVAL = 2.109e-05
MEASURED_LOSS_TRAIN = 6.561e-05
MEASURED_GRAD = {
    "bos_token": 1.055e-03,
    "decoder_mlp.0.weight": 7.679e-04,
    "decoder_mlp.1.weight": 1.062e-03,
    "decoder_mlp.2.weight": 8.660e-04,
    "encoder.encoder.block.0.layer.0.SelfAttention.k.weight": 2.995e-02,
    "encoder.encoder.block.0.layer.0.SelfAttention.o.weight": 2.117e-02,
    "encoder.encoder.block.0.layer.0.SelfAttention.q.weight": 4.102e-02,
    "encoder.encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight": 7.389e-02,
    "encoder.encoder.block.0.layer.0.SelfAttention.v.weight": 2.693e-02,
    "encoder.encoder.block.0.layer.0.layer_norm.weight": 2.265e-02,
    "encoder.encoder.block.0.layer.1.DenseReluDense.wi.weight": 1.380e-01,
    "encoder.encoder.block.0.layer.1.DenseReluDense.wo.weight": 2.295e-03,
    "encoder.encoder.block.0.layer.1.layer_norm.weight": 5.222e-02,
    "encoder.encoder.block.1.layer.0.SelfAttention.k.weight": 8.825e-03,
    "encoder.encoder.block.1.layer.0.SelfAttention.o.weight": 3.484e-03,
    "encoder.encoder.block.1.layer.0.SelfAttention.q.weight": 7.204e-03,
    "encoder.encoder.block.1.layer.0.SelfAttention.v.weight": 2.675e-03,
    "encoder.encoder.block.1.layer.0.layer_norm.weight": 3.994e-03,
    "encoder.encoder.block.1.layer.1.DenseReluDense.wi.weight": 1.567e-02,
    "encoder.encoder.block.1.layer.1.DenseReluDense.wo.weight": 2.993e-03,
    "encoder.encoder.block.1.layer.1.layer_norm.weight": 1.148e-02,
    "encoder.encoder.final_layer_norm.weight": 2.591e-03,
    "item_sid_embedding_table.weight": 3.254e-02,
    "sep_token": 6.764e-03,
    "t5_decoder.block.0.layer.0.SelfAttention.k.weight": 1.297e-03,
    "t5_decoder.block.0.layer.0.SelfAttention.o.weight": 1.065e-03,
    "t5_decoder.block.0.layer.0.SelfAttention.q.weight": 1.505e-03,
    "t5_decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight": 2.352e-03,
    "t5_decoder.block.0.layer.0.SelfAttention.v.weight": 1.722e-03,
    "t5_decoder.block.0.layer.0.layer_norm.weight": 9.393e-04,
    "t5_decoder.block.0.layer.1.EncDecAttention.k.weight": 4.082e-03,
    "t5_decoder.block.0.layer.1.EncDecAttention.o.weight": 1.801e-03,
    "t5_decoder.block.0.layer.1.EncDecAttention.q.weight": 2.885e-03,
    "t5_decoder.block.0.layer.1.EncDecAttention.v.weight": 2.138e-03,
    "t5_decoder.block.0.layer.1.layer_norm.weight": 4.287e-03,
    "t5_decoder.block.0.layer.2.DenseReluDense.wi.weight": 2.430e-03,
    "t5_decoder.block.0.layer.2.DenseReluDense.wo.weight": 1.404e-03,
    "t5_decoder.block.0.layer.2.layer_norm.weight": 1.751e-03,
    "t5_decoder.block.1.layer.0.SelfAttention.k.weight": 3.296e-03,
    "t5_decoder.block.1.layer.0.SelfAttention.o.weight": 2.212e-03,
    "t5_decoder.block.1.layer.0.SelfAttention.q.weight": 3.472e-03,
    "t5_decoder.block.1.layer.0.SelfAttention.v.weight": 1.661e-03,
    "t5_decoder.block.1.layer.0.layer_norm.weight": 1.350e-03,
    "t5_decoder.block.1.layer.1.EncDecAttention.k.weight": 3.074e-03,
    "t5_decoder.block.1.layer.1.EncDecAttention.o.weight": 2.166e-03,
    "t5_decoder.block.1.layer.1.EncDecAttention.q.weight": 3.239e-03,
    "t5_decoder.block.1.layer.1.EncDecAttention.v.weight": 2.465e-03,
    "t5_decoder.block.1.layer.1.layer_norm.weight": 3.753e-03,
    "t5_decoder.block.1.layer.2.DenseReluDense.wi.weight": 1.093e-02,
    "t5_decoder.block.1.layer.2.DenseReluDense.wo.weight": 6.053e-04,
    "t5_decoder.block.1.layer.2.layer_norm.weight": 2.626e-03,
    "t5_decoder.final_layer_norm.weight": 9.358e-04,
    "user_embedding.weight": 2.550e-02,
}
LOSS_EVAL = 4 * MEASURED_LOSS_EVAL
LOSS_TRAIN = 4 * MEASURED_LOSS_TRAIN
GRAD = {name: 4 * value for name, value in MEASURED_GRAD.items()}


@contextlib.contextmanager
def _setting(model, attention, long, arith):
    with impls(model, attention=attention):
        try:
            model.attention_long_impl, model.attention_arith = long, arith
            yield model
        finally:
            model.attention_long_impl, model.attention_arith = "torch", "fp32"


@contextlib.contextmanager
def _spy(monkeypatch):
    """Every fused attention call of the block as (name, Tq, Tk, its `arith` keyword or ABSENT)."""
    import modules.t5 as t5
    calls = []

    def watch(name):
        orig = getattr(t5.ops, name)

        def spied(q, k, *a, **kw):
            calls.append((name, q.shape[1], k.shape[1], kw.get("arith", ABSENT)))
            return orig(q, k, *a, **kw)

        patch.setattr(t5.ops, name, spied)

    with monkeypatch.context() as patch:
        for name in LONG_OPS + SHORT_OPS:
            watch(name)
        yield calls


def _step(model, batch, arith, train, seed):
    """(loss, grads) of one step in eval or train mode (dropout 0.1) on the long kernels in `arith`."""
    try:
        with _setting(model.train() if train else model.eval(), "hip_train", "hip", arith):
            return loss_and_grads(model, batch, seed=seed)
    finally:
        model.eval()


def _differences(seed, train):
    """Relative loss difference and {parameter: max|dg| / max|g_fp32|} of the bf16 arm against the fp32 arm."""
    model, _, batch, _ = _model_and_batch()
    loss32, grads32 = _step(model, batch, "fp32", train, seed)
    loss, grads = _step(model, batch, "bf16", train, seed)
    assert torch.isfinite(loss) and set(grads) == set(grads32)
    assert all(torch.isfinite(g).all() for g in grads.values())
    rel = {n: float((grads[n] - grads32[n]).abs().max() / grads32[n].abs().max()) for n in grads32
           if bool(grads32[n].any())}
    return float((loss - loss32).abs() / loss32.abs()), rel


def measure(seeds=SEEDS):
    """The table of profiles/t5_attention_long_bf16.txt: the largest differences over `seeds`."""
    loss_eval, _ = _differences(None, train=False)
    loss_train, worst = 0.0, {}
    for s in seeds:
        dl, rel = _differences(s, train=True)
        loss_train = max(loss_train, dl)
        for n, r in rel.items():
            worst[n] = max(worst.get(n, 0.0), r)
    return loss_eval, loss_train, worst


def test_every_long_call_carries_the_arithmetic_and_no_short_call_does(monkeypatch):
    model, _, batch, _ = _model_and_batch()
    with _setting(model.eval(), "hip_train", "hip", "bf16"), _spy(monkeypatch) as calls:
        loss_and_grads(model, batch)
        n_train = len(calls)
        with torch.no_grad():
            torch.manual_seed(7)
            model.generate_next_sem_id(batch)
    seen = {name: [c for c in calls if c[0] == name] for name in LONG_OPS + SHORT_OPS}
    assert len(seen["t5_attention_long_fwd_train"]) == 2 * LAYERS and len(seen["t5_attention_long_bwd"]) == 2 * LAYERS
    assert len(seen["t5_attention_long"]) == LAYERS + LAYERS * L          # generate: the encoder and the cross-attention
    assert sum(1 for c in calls[n_train:] if c[:3] == ("t5_attention_long", 1, T_ENC)) == LAYERS * L
    for name in LONG_OPS:
        assert all(c[3] == "bf16" for c in seen[name]), name
    for name in SHORT_OPS:
        assert seen[name] and all(c[3] == ABSENT for c in seen[name]), name


def test_default_attribute_passes_no_keyword(monkeypatch):
    model, _, batch, _ = _model_and_batch()
    assert model.attention_arith == "fp32"
    with _setting(model.eval(), "hip_train", "hip", "fp32"), _spy(monkeypatch) as calls:
        loss_and_grads(model, batch)
        with torch.no_grad():
            torch.manual_seed(7)
            model.generate_next_sem_id(batch)
    assert sum(1 for c in calls if c[0] in LONG_OPS) == 4 * LAYERS + LAYERS + LAYERS * L
    assert all(c[3] == ABSENT for c in calls)


def test_eval_loss_against_the_fp32_arm():
    dl, _ = _differences(None, train=False)
    print(f"eval-mode loss: relative difference {dl:.3e} (threshold {LOSS_EVAL:.3e})")
    assert dl < SANITY_CAP
    assert dl <= LOSS_EVAL


def test_train_mode_step_against_the_fp32_arm():
    model, _, batch, _ = _model_and_batch()
    assert model.t5_decoder.config.dropout_rate == 0.1
    dl, rel = _differences(SEEDS[0], train=True)
    print(f"train-mode loss: relative difference {dl:.3e} (threshold {LOSS_TRAIN:.3e})")
    assert dl < SANITY_CAP
    assert dl <= LOSS_TRAIN
    assert set(rel) <= set(GRAD)
    for n in sorted(rel):
        print(f"  {n}: max|dg| / max|g_fp32| {rel[n]:.3e} (threshold {GRAD[n]:.3e})")
    for n, r in rel.items():
        assert r <= GRAD[n], (n, r)
    # the same seed gives the same bits
    loss_a, grads_a = _step(model, batch, "bf16", True, SEEDS[0])
    loss_b, grads_b = _step(model, batch, "bf16", True, SEEDS[0])
    assert same_bits(loss_a.reshape(1), loss_b.reshape(1)) and all(same_bits(grads_a[n], grads_b[n]) for n in grads_a)


def test_generate_runs_on_the_bf16_arm():
    model, _, batch, _ = _model_and_batch()
    k = model.top_k_for_generation
    outs = {}
    for arith in ("fp32", "bf16"):
        with _setting(model.eval(), "hip", "hip", arith):
            torch.manual_seed(7)
            outs[arith] = model.generate_next_sem_id(batch)
    out, ref = outs["bf16"], outs["fp32"]
    assert out.sem_ids.shape == ref.sem_ids.shape == (B, k, L) and out.log_probas.shape == ref.log_probas.shape == (B, k)
    lp = out.log_probas
    assert bool(torch.isfinite(lp).all()) == bool(torch.isfinite(ref.log_probas).all())
    finite = torch.isfinite(lp)
    assert bool(finite.any())
    assert bool((lp[:, :-1] >= lp[:, 1:])[finite[:, 1:]].all())            # descending per row
    # beams may flip on near ties: ids are not compared
    try:
        model.attention_arith = "fp16"
        with pytest.raises(ValueError, match="attention_arith"):
            model.generate_next_sem_id(batch)
        with pytest.raises(ValueError, match="attention_arith"):
            model(batch)
    finally:
        model.attention_arith = "fp32"
