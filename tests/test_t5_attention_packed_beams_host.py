"""The host side of the packed beams' cross-attention and of packed rows in `generate` (include/rqhip.h:
rqhip_t5_attention_packed_beams; modules/model.py; evaluate_decoder.py, recommend.py).  No GPU needed.

The C entry point is called with null or small fake addresses that nothing dereferences (16: aligned), as in
tests/test_t5_attention_calls_host.py: every case ends in a check that fails, before any device call, and the message
names the argument."""
import inspect
import os
import re

import pytest

from conftest import ROOT

NAME = "rqhip_t5_attention_packed_beams"
ARGS = "q ld_q k v ld_kv R Rk n_k H d_kv Tq Tk cu_k out ld_out"
# four groups of at most 8 keys, three beams each, 20 packed keys; q, k, v and out stay null: the checks look at them last
DEFAULTS = dict(q=None, ld_q=128, k=None, v=None, ld_kv=128, R=12, Rk=4, n_k=20, H=2, d_kv=64, Tq=1, Tk=8, cu_k=16,
                out=None, ld_out=128)
EARG, EUNSUPPORTED = -1, -2


def _call(**overrides):
    from rqhip import _lib
    l = _lib.lib()
    values = dict(DEFAULTS, **overrides)
    rc = getattr(l, NAME)(*[values[name] for name in ARGS.split()], None)
    return rc, l.rqhip_last_error().decode()


def test_the_symbol_is_declared_exported_and_bound():
    import ctypes

    from rqhip import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rqhip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", text)
    assert hasattr(ctypes.CDLL(_lib.SO_PATH), NAME)
    res, args = _lib.SIGNATURES[NAME]
    assert res is ctypes.c_int and len(args) == len(ARGS.split()) + 1           # and the stream
    assert _lib.lib().rqhip_version() == 462


def test_error_codes_are_those_of_the_header():
    text = open(os.path.join(ROOT, "include", "rqhip.h")).read()
    assert int(re.search(r"#define\s+RQHIP_EARG\s+\(?(-?\d+)", text).group(1)) == EARG
    assert int(re.search(r"#define\s+RQHIP_EUNSUPPORTED\s+\(?(-?\d+)", text).group(1)) == EUNSUPPORTED


@pytest.mark.parametrize("case, overrides, code, names", [
    ("null cu_k", dict(cu_k=None), EARG, "cu_k"),
    ("R % Rk != 0", dict(R=13), EARG, "Rk="),
    ("Tk = 257", dict(Tk=257), EUNSUPPORTED, "Tk=257"),
    ("n_k > Rk * Tk", dict(n_k=33), EARG, "n_k=33"),
    ("n_k beyond int32", dict(n_k=2 ** 31, Rk=2 ** 29, R=2 ** 29), EARG, "n_k="),
    ("a stride that is no multiple of 4", dict(ld_kv=130), EARG, "k/v 130"),
    ("a q stride that is no multiple of 4", dict(ld_q=130), EARG, "q 130"),
    ("too many query rows per group", dict(q=16, k=16, v=16, out=16, R=2 ** 24, Rk=1, n_k=8), EUNSUPPORTED,
     "16777216 query rows"),
    ("null q", {}, EARG, "null pointer"),
    ("misaligned", dict(q=8, k=8, v=8, out=8), EARG, "16-byte aligned"),
])
def test_the_entry_point_rejects_before_any_device_call(case, overrides, code, names):
    rc, msg = _call(**overrides)
    assert rc == code and rc < 0, (case, rc, msg)            # negative: an argument error, never a HIP error
    assert msg.startswith("t5_attention_packed_beams: ") and names in msg, (case, msg)


def test_nothing_to_do_returns_ok():
    assert _call(R=0, Rk=0, n_k=0)[0] == 0


@pytest.mark.parametrize("entry", ["evaluate", "recommend"])
def test_entry_points_validate_the_binding_first(entry):
    """A bad encoder_rows.mode raises before the checkpoint, the data or the GPU are looked at."""
    import evaluate_decoder
    import recommend
    import train_decoder
    fn = {"evaluate": evaluate_decoder.evaluate, "recommend": recommend.recommend}[entry]
    assert evaluate_decoder.encoder_rows is train_decoder.encoder_rows is recommend.encoder_rows    # one configurable
    gin = train_decoder.gin
    gin.clear_config()
    try:
        gin.parse_config('encoder_rows.mode = "ragged"')
        with pytest.raises(ValueError, match="encoder_rows"):
            fn(checkpoint_path="no such checkpoint.pt", dataset=train_decoder.RecDataset.AMAZON,
               dataset_folder="no such folder")
        with pytest.raises(ValueError, match="encoder_rows"):
            fn()
    finally:
        gin.clear_config()
    assert train_decoder.encoder_rows() == "padded"


def test_generate_takes_item_counts():
    from modules.model import EncoderDecoderRetrievalModel
    p = inspect.signature(EncoderDecoderRetrievalModel.generate).parameters
    assert list(p) == ["self", "attention_mask", "input_ids", "user_id", "item_counts"]
    assert p["item_counts"].kind is inspect.Parameter.KEYWORD_ONLY and p["item_counts"].default is None


@pytest.mark.parametrize("base, packed", [("decoder_amazon_eval.gin", "decoder_amazon_eval_packed.gin"),
                                          ("decoder_amazon_recommend.gin", "decoder_amazon_recommend_packed.gin")])
def test_packed_configs_are_the_base_configs_plus_one_line(base, packed):
    cfg = os.path.join(ROOT, "rq-vae-recommender_amd", "configs")

    def bindings(name):
        return [l.strip() for l in open(os.path.join(cfg, name)) if l.strip() and not l.startswith("#")]

    assert [l for l in bindings(packed) if l not in bindings(base)] == ['encoder_rows.mode="packed"']
    assert [l for l in bindings(base) if l not in bindings(packed)] == []
