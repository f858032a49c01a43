"""The five forms (ops.T5MatmulForm) of the "hip" feed-forward and grouped projections on the retrieval model: for every
form and for a train step under grad, an eval forward under no_grad and a `generate` on a decode cache, ONLY the C entry
points with the form's suffix run, as often as the block structure says; the weight images are refreshed once per stack
and not again; and the four "bf16" forms give one another's bits.

The model is tiny_model(32, 32): one block per stack, three hierarchy levels.  Per forward that is one feed-forward
call per block of each stack, two projection calls per self-attention (q, k, v and o), two per cross-attention (q and
o) and one grouped cross-attention K/V call per four decoder blocks:

    forward (encoder + decoder)  feed-forward 1 + 1, projections 2 + (2 + 2 + 1)
    generate                     the encoder (1, 2), the K/V call (0, 1) and one decoder step per level, its K/V given (1, 4)

Under grad every forward call has one backward call.  Saved activations exist only under grad: under no_grad a `saved`
form runs the entry points of its twin without them.  There is no tolerance in this file."""
import functools
import re

import pytest
import torch

from retrieval_cases import loss_and_grads, same_bits
from test_gpu_t5_saved_activations import _batch, _model

pytestmark = pytest.mark.gpu

# form -> (matmul_arith, weight_images, saved_activations), the entry suffix, the suffix under no_grad
FORMS = {"T5_FP32": (("fp32", "none", "fp32"), "", ""),
         "T5_BF16": (("bf16", "none", "fp32"), "_bf16", "_bf16"),
         "T5_BF16_IMAGES": (("bf16", "bf16", "fp32"), "_bf16w", "_bf16w"),
         "T5_BF16_SAVED": (("bf16", "none", "bf16"), "_bf16a", "_bf16"),
         "T5_BF16_IMAGES_SAVED": (("bf16", "bf16", "bf16"), "_bf16wa", "_bf16w")}
MODES = ("train", "eval", "generate")
LEVELS = 3
# mode -> calls of (t5_ffn_fwd, t5_proj_fwd); a backward for each under grad
FORWARD_CALLS = {"train": (2, 7), "eval": (2, 7), "generate": (1 + LEVELS, 2 + 1 + 4 * LEVELS)}


def _entries():
    """The launching entry points of the two kernels: rqhip_t5_{ffn,proj}_{fwd,bwd} with every suffix."""
    from rqhip import _lib
    names = [n for n in _lib.SIGNATURES if re.fullmatch(r"rqhip_t5_(ffn|proj)_(fwd|bwd)(_bf16(w|a|wa)?)?", n)]
    assert len(names) == 2 * 5 + 2 * 3
    return names


def _count(monkeypatch):
    """Every call of those entry points, counted at the library handle the ops look them up on."""
    from rqhip import _lib
    handle = _lib.lib()
    calls = dict.fromkeys(_entries(), 0)
    for name in calls:
        def counted(*a, _name=name, _real=getattr(handle, name)):
            calls[_name] += 1
            return _real(*a)
        monkeypatch.setattr(handle, name, counted)
    return calls


def _expected(form, mode):
    _, suffix, suffix_no_grad = FORMS[form]
    ffn, proj = FORWARD_CALLS[mode]
    want = dict.fromkeys(_entries(), 0)
    if mode == "train":
        want.update({f"rqhip_t5_ffn_fwd{suffix}": ffn, f"rqhip_t5_ffn_bwd{suffix}": ffn})
        proj_suffix = suffix.replace("a", "")       # the projections save no activations
        want.update({f"rqhip_t5_proj_fwd{proj_suffix}": proj, f"rqhip_t5_proj_bwd{proj_suffix}": proj})
    else:
        want.update({f"rqhip_t5_ffn_fwd{suffix_no_grad}": ffn, f"rqhip_t5_proj_fwd{suffix_no_grad}": proj})
    return want


def _form_model(form, mode):
    (arith, images, saved), _, _ = FORMS[form]
    m = _model(saved, images == "bf16", arith=arith)
    assert (m.attention_impl, m.norm_impl, m.head_impl, m.ffn_impl, m.proj_impl) == ("hip_train", "hip", "hip", "hip", "hip")
    assert len(m.encoder.encoder.block) == len(m.t5_decoder.block) == 1 and m.num_hierarchies == LEVELS
    if mode == "generate":
        m.attention_impl, m.beam_impl = "hip", "exact"
    return m.train() if mode == "train" else m.eval()


def _run(m, mode):
    """One pass of `mode` -> its results as a flat list of tensors."""
    batch = _batch(1)
    if mode == "train":
        loss, grads = loss_and_grads(m, batch, seed=3)
        assert len(grads) > 20
        return [loss] + [grads[n] for n in sorted(grads)]
    if mode == "eval":
        with torch.no_grad():
            return [m(batch).loss]
    out = m.generate_next_sem_id(batch)
    return [out.sem_ids, out.log_probas]


@functools.lru_cache(maxsize=None)
def _bf16_results(mode):
    """What the plain "bf16" form gives, computed once and left unchanged."""
    return _run(_form_model("T5_BF16", mode), mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", list(FORMS))
def test_only_the_entries_of_the_form_run(monkeypatch, form, mode):
    import modules.t5 as t5
    from rqhip import ops
    (arith, images, saved), suffix, _ = FORMS[form]
    assert getattr(ops, form) == (arith, images == "bf16", saved == "bf16")
    want_bits = _bf16_results(mode) if arith == "bf16" else None      # before the counting starts
    m = _form_model(form, mode)
    stacks = (m.encoder.encoder, m.t5_decoder)
    caches = []
    real_cache = t5.T5Stack.new_decode_cache
    monkeypatch.setattr(t5.T5Stack, "new_decode_cache", lambda self, *a: caches.append(real_cache(self, *a)) or caches[-1])
    calls = _count(monkeypatch)
    got = _run(m, mode)
    assert calls == _expected(form, mode)
    assert len(caches) == (1 if mode == "generate" else 0)
    # the images: one refresh launch per stack for new weights, none for the same weights again
    refreshes = [1, 1] if images == "bf16" and arith == "bf16" else [0, 0]
    assert [s.images.refreshes for s in stacks] == refreshes
    again = _run(m, mode)
    assert [s.images.refreshes for s in stacks] == refreshes
    assert calls == {name: 2 * n for name, n in _expected(form, mode).items()}
    assert len(again) == len(got) and all(same_bits(a, b) for a, b in zip(again, got))
    if want_bits is not None:
        assert len(got) == len(want_bits) and all(same_bits(a, b) for a, b in zip(got, want_bits))
