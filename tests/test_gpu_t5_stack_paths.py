"""The one block loop of T5Stack.forward (modules/t5.py) under all 12 settings of (attention_impl, norm_impl, ffn_impl):
the encoder's and the decoder's hidden states of the small model of tests/test_gpu_t5_ffn_impl.py under no_grad in eval
mode, gated as there against the fp64 model relative to the all-operator fp32 error (factor 4), and the number of fused
attention launches each setting makes."""
import functools
import itertools

import pytest
import torch

from retrieval_cases import LAYERS, gate, impls, small_model

pytestmark = pytest.mark.gpu

SMALL = (12, 96, False)         # the set-up of tests/test_gpu_t5_ffn_impl.py


def _hidden_states(model, batch, launches=()):
    """(encoder output, decoder output, len(launches) after the encoder) of `batch`, as model.forward computes them."""
    from modules.model import _strip_dedup_col
    L = model.num_hierarchies
    with torch.no_grad():
        enc, enc_mask = model.encoder_forward_pass(attention_mask=_strip_dedup_col(batch.seq_mask.long(), L + 1, L),
                                                   input_ids=_strip_dedup_col(batch.sem_ids, L + 1, L),
                                                   user_id=batch.user_ids)
        n_enc = len(launches)
        dec = model.decoder_forward_pass(future_ids=batch.sem_ids_fut[:, :L], encoder_output=enc,
                                         attention_mask_for_encoder=enc_mask)
    return enc, dec, n_enc


@functools.lru_cache(maxsize=None)
def _references():
    """The hidden states of the fp64 model on the CPU and of the all-operator fp32 model on the device."""
    model, model64, batch, batch64 = small_model(*SMALL)
    with impls(model.eval()):
        return _hidden_states(model64, batch64)[:2], _hidden_states(model, batch)[:2]


@pytest.mark.parametrize("attention,norm,ffn", list(itertools.product(("torch", "hip", "hip_train"), ("torch", "hip"),
                                                                      ("torch", "hip"))))
def test_hidden_states_and_attention_launches(attention, norm, ffn, monkeypatch):
    import modules.t5 as t5
    model, _, batch, _ = small_model(*SMALL)
    (enc64, dec64), (enc32, dec32) = _references()
    calls = []
    orig = t5.ops.t5_attention

    def counted(*a, **kw):
        calls.append(1)
        return orig(*a, **kw)

    monkeypatch.setattr(t5.ops, "t5_attention", counted)
    with impls(model.eval(), attention=attention, norm=norm, ffn=ffn):
        enc, dec, n_enc = _hidden_states(model, batch, calls)
    assert enc.shape == enc32.shape and dec.shape == dec32.shape == (3, 4, 64)
    fused = attention != "torch"
    assert (n_enc, len(calls) - n_enc) == ((LAYERS, 2 * LAYERS) if fused else (0, 0))
    gate(f"{attention}/{norm}/{ffn} encoder", enc, enc32, enc64, 4)
    gate(f"{attention}/{norm}/{ffn} decoder", dec, dec32, dec64, 4)
