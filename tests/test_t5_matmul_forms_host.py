"""The forms of the "hip" feed-forward and grouped projections on the host: `modules.t5.matmul_forms` against a table
written out here, the entry point each form resolves to in rqhip.ops (no library loaded), and the validation of the nine
stack attributes by a stack and by the model.  No GPU needed."""
import itertools
import re

import pytest
import torch

from retrieval_cases import tiny_batch, tiny_model

F32, B16, B16W, B16A, B16WA = "T5_FP32", "T5_BF16", "T5_BF16_IMAGES", "T5_BF16_SAVED", "T5_BF16_IMAGES_SAVED"
# (matmul_arith, weight_images, saved_activations) -> the feed-forward's form under grad, under no_grad, the projections'
TABLE = {("fp32", "none", "fp32"): (F32, F32, F32),
         ("fp32", "none", "bf16"): (F32, F32, F32),
         ("fp32", "bf16", "fp32"): (F32, F32, F32),
         ("fp32", "bf16", "bf16"): (F32, F32, F32),
         ("bf16", "none", "fp32"): (B16, B16, B16),
         ("bf16", "none", "bf16"): (B16A, B16, B16),
         ("bf16", "bf16", "fp32"): (B16W, B16W, B16W),
         ("bf16", "bf16", "bf16"): (B16WA, B16W, B16W)}
SUFFIX = {F32: "", B16: "_bf16", B16W: "_bf16w", B16A: "_bf16a", B16WA: "_bf16wa"}


def test_matmul_forms_over_all_inputs():
    from modules.t5 import MATMUL_ARITHS, SAVED_ACTIVATIONS, WEIGHT_IMAGES, matmul_forms
    from rqhip import ops
    assert len(TABLE) == 8 and set(TABLE) == set(itertools.product(MATMUL_ARITHS, WEIGHT_IMAGES, SAVED_ACTIVATIONS))
    seen, n = set(), 0
    for attrs, (ffn_grad, ffn_no_grad, proj) in TABLE.items():
        for ffn_active, proj_active, grad in itertools.product((False, True), repeat=3):
            got_ffn, got_proj = matmul_forms(*attrs, ffn_active, proj_active, grad)
            want_ffn = getattr(ops, ffn_grad if grad else ffn_no_grad) if ffn_active else None
            want_proj = getattr(ops, proj) if proj_active else None
            assert got_ffn == want_ffn and got_proj == want_proj, (attrs, ffn_active, proj_active, grad)
            assert got_proj is None or not got_proj.saved
            assert grad or got_ffn is None or not got_ffn.saved
            seen |= {f for f in (got_ffn, got_proj) if f is not None}
            n += 1
    assert n == 64
    assert seen == {getattr(ops, name) for name in SUFFIX} and len(seen) == 5
    for form in seen:
        assert isinstance(form, ops.T5MatmulForm) and type(form.images) is bool and type(form.saved) is bool
    with pytest.raises(AttributeError):
        ops.T5_FP32.arith = "bf16"          # immutable


def test_each_form_resolves_to_the_entry_point_with_its_suffix(monkeypatch):
    from rqhip import _lib, ops

    class Names:                 # every attribute is its own name: no library is loaded
        def __getattr__(self, name):
            return name

    monkeypatch.setattr(_lib, "lib", lambda: Names())
    images = [object()]
    for name, suffix in SUFFIX.items():
        form = getattr(ops, name)
        for who in ("t5_ffn_fwd", "t5_ffn_bwd", "t5_proj_fwd", "t5_proj_bwd"):
            if form.saved and "proj" in who:
                continue
            kw = form.keywords(images)
            assert kw.get("w_images") is (images if form.images else None)
            got = ops.t5_matmul_entry(who, **kw)
            assert got == (form, f"rqhip_{who}{suffix}", f"rqhip_{who}{suffix}"), (name, who)
    assert ops.T5_FP32.keywords() == {}      # the plain call
    # the complaints, in their order: an unknown arithmetic, images off "bf16", saved activations off "bf16"
    for kw, text in (({"arith": "fp16", "w_images": images, "saved": "bf16"}, "arith must be one of"),
                     ({"arith": "fp32", "w_images": images, "saved": "bf16"}, 'w_images belong to arith="bf16"'),
                     ({"arith": "fp32", "saved": "bf16"}, 'saved="bf16" belongs to arith="bf16"'),
                     ({"arith": "bf16", "saved": "fp16"}, "saved must be one of")):
        with pytest.raises(_lib.RqHipError, match=text):
            ops.t5_matmul_entry("t5_ffn_fwd", **kw)


BAD = "bogus"


def test_every_attribute_is_validated_by_a_stack_and_by_the_model():
    from modules.t5 import STACK_ATTRIBUTES, T5Config, T5Stack
    assert list(STACK_ATTRIBUTES) == ["attention_impl", "attention_long_impl", "norm_impl", "ffn_impl", "proj_impl",
                                      "matmul_arith", "attention_arith", "weight_images", "saved_activations"]
    stack = T5Stack(T5Config(16, d_model=32, num_heads=2, d_ff=64, num_layers=1)).eval()
    decoder = T5Stack(T5Config(16, d_model=32, num_heads=2, d_ff=64, num_layers=1, is_decoder=True)).eval()
    m = tiny_model(32, 32).eval()
    x = torch.randn(2, 3, 32)
    for name, allowed in STACK_ATTRIBUTES.items():
        text = re.escape(f"{name} must be one of {allowed}, got {BAD!r}")
        good = getattr(stack, name)
        assert good == allowed[0] == getattr(m, name)
        for owner, call in ((stack, lambda: stack(x)), (decoder, lambda: decoder.cross_kv(x)), (m, lambda: m(tiny_batch())),
                            (m, m._push_attention_impl)):
            setattr(owner, name, BAD)
            with pytest.raises(ValueError, match=text):
                call()
            setattr(owner, name, good)
    with torch.no_grad():       # and with every value put back, all of them run
        stack(x), decoder.cross_kv(x), m(tiny_batch())
