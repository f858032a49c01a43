"""One train-mode step of the retrieval model on its fused paths, dropout active, against the operator model in fp64 with
the same masks (retrieval_cases.record_step / replay_step).

The kernels' dropout decision is a published function of (seed, element index, p) (include/rqhip.h,
ops.t5_attention_dropout_keep), so the masks a fused step used are rebuilt from the seeds, rates and shapes its ops calls
received, logged in the order of the forward, and handed one by one to torch.nn.functional.dropout of the all-operator
model: once in fp32 on the device (e_torch) and once in fp64 on the host (the reference).  What this sees and the
kernels' own tests cannot: a dropout site missing, doubled or at the wrong rate on a fused path (the replay fails with
the site's index, or the gate does), a backward given another seed, rate or extent than its forward, a seed handed to
two calls, dropout taken in eval mode.

Model: retrieval_cases.small_model(12, 96, True) -- d_model 64, 2 heads, d_ff 96, 2 layers, batch 3 with a padded row,
encoder T = 8, decoder T = 4, norm weights perturbed -- at its own dropout rate 0.1.  Settings (attention, norm, ffn,
head, embed, proj): everything fused; train_decoder.py's (the projections on the operators); the fused attention, the
fused glue, the fused feed-forward alone (in the last, each feed-forward draws its own seed between operator dropouts);
and everything fused on a history of 6 items: encoder T = 24, so the attention forward and backward take their
instantiation for more than 16 keys, and the glue and the feed-forward see several 16-row tiles per stack.

Gates: retrieval_cases.gate, e = max|a - a64| / max|a64| per tensor, e_kernel <= max(4 e_torch, 2^-22) for the loss and
max(8 e_torch, 2^-22) for every parameter gradient, the factors of the eval-mode model tests.  A gradient whose fp64
reference is exactly zero must be exactly zero.  Measured ratios: profiles/train_mode_replay.txt."""
import functools

import pytest
import torch

from retrieval_cases import LAYERS, gate, loss_and_grads, record_step, recording, replay_step, setting, small_model

pytestmark = pytest.mark.gpu

SMALL = (12, 96, True)
STEP_SEED, DRAW_SEED = 21, 5
FUSED = dict(attention="hip_train", norm="hip", ffn="hip", head="hip", embed="hip", proj="hip")
SETTINGS = {                                        # name -> (the choices, items of the history)
    "fused": (FUSED, 2),
    "train_decoder": ({**FUSED, "proj": "torch"}, 2),
    "attention": (dict(attention="hip_train"), 2),
    "glue": (dict(norm="hip"), 2),
    "ffn": (dict(ffn="hip"), 2),
    "fused, 6 items": (FUSED, 6),
}
SITES = (2 + 4 * LAYERS) + (2 + 6 * LAYERS)         # per stack: the embeddings, the final norm's output, the blocks'
CALLS = {"attention": 3 * LAYERS, "glue": (2 * LAYERS + 1) + (3 * LAYERS + 1), "ffn": 2 * LAYERS}


def _models(name):
    items = SETTINGS[name][1]
    return small_model(*SMALL) if items == 2 else small_model(*SMALL, items=items)


@functools.lru_cache(maxsize=None)
def _step(name):
    """(loss, gradients, log) of one fused step, and (loss, gradients) of its replay in fp32 and in fp64."""
    model, model64, batch, batch64 = _models(name)
    with setting(model.eval(), **SETTINGS[name][0]):
        loss, grads, log = record_step(model, batch, seed=STEP_SEED, draw_seed=DRAW_SEED)
    with setting(model):
        ref32 = replay_step(model, batch, log)
    ref64 = replay_step(model64, batch64, log)
    assert not model.training and not model64.training
    return loss, grads, log, ref32, ref64


def _kinds(choices):
    """The kinds of the sites of one step in the order of the forward (modules/t5.py)."""
    a = "attention" if choices.get("attention") == "hip_train" else "operator"
    g_in, g_out = ("glue_in", "glue_out") if choices.get("norm") == "hip" else ("operator", "operator")
    f = "ffn" if choices.get("ffn") == "hip" else "operator"
    kinds = []
    for decoder in (False, True):
        kinds.append(g_in)
        for _ in range(LAYERS):
            kinds += [a, g_in] * (2 if decoder else 1) + [f, g_in]
        kinds.append(g_out)
    return kinds


def _expected_calls(choices):
    on = {"attention": choices.get("attention") == "hip_train", "glue": choices.get("norm") == "hip",
          "ffn": choices.get("ffn") == "hip"}
    return {op: CALLS[op] if on[op] else 0 for op in CALLS}


def _counts(calls):
    return {op: sum(c.op == op for c in calls) for op in CALLS}


@pytest.mark.parametrize("name", list(SETTINGS))
def test_loss_and_gradients_against_fp64_with_the_step_s_own_masks(name):
    loss, grads, log, (loss32, grads32), (loss64, grads64) = _step(name)
    choices = SETTINGS[name][0]
    # the replays consumed the whole log (replaying raises otherwise); every site where and of the kind it belongs
    assert len(log) == SITES and [s.kind for s in log.sites] == _kinds(choices)
    assert all(s.p == 0.1 for s in log.sites)
    assert _counts(log.fused("fwd")) == _counts(log.fused("bwd")) == _expected_calls(choices)
    assert sorted(grads) == sorted(grads32) == sorted(grads64) and len(grads) > 40
    gate(f"{name}: loss", loss.reshape(1), loss32.reshape(1), loss64.reshape(1), 4)
    for n in sorted(grads):
        gate(f"{name}: grad {n}", grads[n], grads32[n], grads64[n], 8)


@pytest.mark.parametrize("name", ["fused", "ffn"])
def test_seeds_rates_and_shapes_of_the_fused_calls(name):
    """Every forward call got a seed of its own; each backward call got its forward's seed, rates and shapes."""
    log = _step(name)[2]
    fwd, bwd = log.fused("fwd"), log.fused("bwd")
    assert len(fwd) == len(bwd) == sum(_expected_calls(SETTINGS[name][0]).values()) > 0
    assert all(c.seed is not None for c in fwd)
    by_seed = {c.seed: c for c in fwd}
    assert len(by_seed) == len(fwd), "two fused calls of one step share a seed"
    assert sorted(c.seed for c in bwd) == sorted(by_seed)
    for c in bwd:
        f = by_seed[c.seed]
        assert (c.op, c.p, c.shapes) == (f.op, f.p, f.shapes), (c, f)
    # the rates: 0.1 everywhere, the second one of the glue in the last call of each stack alone
    glue = [c for c in fwd if c.op == "glue"]
    last = {2 * LAYERS, len(glue) - 1}
    assert all(c.p == ((0.1, 0.1) if k in last else (0.1, 0.0)) for k, c in enumerate(glue))
    assert all(c.p == (0.1,) for c in fwd if c.op != "glue")
    # each site's mask came from a fused call's seed, the two sites of a final glue from one
    seeds = [s.seed for s in log.sites if s.kind != "operator"]
    assert len(set(seeds)) == len(fwd) and set(seeds) == set(by_seed)


@pytest.mark.parametrize("name", ["fused", "ffn"])
def test_eval_mode_under_grad_drops_nothing_and_draws_no_seed(name):
    model, _, batch, _ = _models(name)
    with setting(model.eval(), **SETTINGS[name][0]), recording() as log:
        state = torch.cuda.get_rng_state()
        loss, grads = loss_and_grads(model, batch)
        assert torch.equal(torch.cuda.get_rng_state(), state)
    assert torch.isfinite(loss) and len(grads) > 40
    assert len(log) == 0
    assert _counts(log.fused("fwd")) == _counts(log.fused("bwd")) == _expected_calls(SETTINGS[name][0])
    assert all(c.seed is None and not any(c.p) for c in log.calls)


def test_a_glue_mask_of_another_seed_in_the_reference_fails_the_gate():
    """The control, on the reference's side only: the fused step of "fused" as it was, the operator replays with the
    mask of one glue site (the one behind the decoder's first cross-attention) rebuilt from another seed.  Against that
    reference the fused gradients must miss the gate, or the gate could not tell a wrong mask from rounding."""
    from test_gpu_t5_add_norm import _masks
    model, model64, batch, batch64 = _models("fused")
    _, grads, log, _, _ = _step("fused")
    i = (2 + 4 * LAYERS) + 4
    s = log.sites[i]
    assert s.kind == "glue_in" and log.sites[i - 1].kind == "attention"
    N, d = s.keep.numel() // s.keep.shape[-1], s.keep.shape[-1]
    keep = _masks(s.seed + 1, N, d, s.p, 0.0)[0].view(s.keep.shape).to(s.keep.device)
    assert not torch.equal(keep, s.keep)
    wrong = log.swapped(i, keep)
    with setting(model.eval()):
        _, grads32 = replay_step(model, batch, wrong)
    _, grads64 = replay_step(model64, batch64, wrong)
    missed = []
    for n in sorted(grads):
        try:
            gate(f"site {i} of another seed: grad {n}", grads[n], grads32[n], grads64[n], 8)
        except AssertionError:
            missed.append(n)
    print(f"{len(missed)} of {len(grads)} gradients miss the gate against the wrong reference")
    assert missed
