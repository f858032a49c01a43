"""The retrieval model (modules/model.py) on the host: state-dict layout, forward / gradients against the reference's
recorded values (tests/golden/retrieval_*.npz, tools/gen_retrieval_golden.py), the beam step's argument checks and the
k > n_cands error.  No GPU needed."""
import pytest
import torch

from conftest import load_golden
from retrieval_cases import CASES, build_model, check_forward, fixture_batch


def test_state_dict_names_shapes_and_strict_load():
    from modules.model import EncoderDecoderRetrievalModel
    fx = load_golden("retrieval_state_dict.npz")
    torch.manual_seed(0)
    model = EncoderDecoderRetrievalModel(torch.zeros(10, 4, dtype=torch.long), 3, 256)
    sd = model.state_dict()
    assert list(sd.keys()) == [str(n) for n in fx["names"]]
    for (name, v), shape in zip(sd.items(), fx["shapes"]):
        assert tuple(v.shape) == tuple(int(s) for s in shape if s >= 0), name
    assert sum(p.numel() for p in model.parameters()) == int(fx["n_params"]) == 4853120
    # a second instance loads the first one's checkpoint strictly
    other = EncoderDecoderRetrievalModel(torch.zeros(10, 4, dtype=torch.long), 3, 256)
    other.load_state_dict(sd, strict=True)
    assert torch.equal(other.t5_decoder.block[0].layer[1].EncDecAttention.k.weight,
                       model.t5_decoder.block[0].layer[1].EncDecAttention.k.weight)
    # the encoder's stack reads the shared table, as in T5EncoderModel
    assert model.encoder.encoder.embed_tokens is model.encoder.shared


@pytest.mark.parametrize("case", CASES)
def test_forward_and_gradients_match_reference_cpu(case):
    fx = load_golden(f"retrieval_{case}.npz")
    torch.manual_seed(0)
    check_forward(fx, build_model(fx), fixture_batch(fx))


def test_strip_dedup_col_and_offsets():
    from modules.model import EncoderDecoderRetrievalModel, _strip_dedup_col
    t = torch.arange(2 * 8).view(2, 8)  # 2 items of 3 ids + dedup
    assert _strip_dedup_col(t, 4, 3).tolist() == [[0, 1, 2, 4, 5, 6], [8, 9, 10, 12, 13, 14]]
    m = EncoderDecoderRetrievalModel(torch.zeros(4, 3, dtype=torch.long), 3, 16, t5_d_model=8, t5_num_heads=1,
                                     t5_d_ff=8, t5_num_layers=1)
    ids = torch.tensor([[1, 2, 3, -1, -1, -1]])
    mask = torch.tensor([[1, 1, 1, 0, 0, 0]])
    assert m._add_repeating_offset_to_rows(ids, 16, 3, mask).tolist() == [[1, 18, 35, 0, 0, 0]]


def test_generate_rejects_k_above_n_cands_before_touching_the_device():
    from modules.model import EncoderDecoderRetrievalModel
    m = EncoderDecoderRetrievalModel(torch.zeros(4, 3, dtype=torch.long), 3, 8, t5_d_model=8, t5_num_heads=1,
                                     t5_d_ff=8, t5_num_layers=1, top_k_for_generation=9)
    with pytest.raises(ValueError, match="n_cands"):
        m.generate(torch.ones(1, 3, dtype=torch.long), torch.zeros(1, 3, dtype=torch.long))


def test_generate_on_cpu_raises_rqhip_error():
    from modules.model import EncoderDecoderRetrievalModel
    from rqhip._lib import RqHipError
    m = EncoderDecoderRetrievalModel(torch.zeros(4, 3, dtype=torch.long), 3, 8, t5_d_model=8, t5_num_heads=1,
                                     t5_d_ff=8, t5_num_layers=1, top_k_for_generation=4)
    with pytest.raises(RqHipError):
        m.generate(torch.ones(1, 3, dtype=torch.long), torch.zeros(1, 3, dtype=torch.long))


def _beam(l, *, h=0, B=4, beams_in=1, K=256, n=64, k=10, H=3, N=0, ld_logits=None, parents=False):
    return l.rqhip_beam_step(None, K if ld_logits is None else ld_logits, None, 1 if parents else None,
                             1 if parents else None, h, B, beams_in, K, n, k, None, 0, None, N, H, H, None, None, None,
                             None, 0, None)


def test_beam_step_argument_checks_without_gpu():
    from rqhip import _lib
    l = _lib.lib()
    assert l.rqhip_beam_step_workspace_bytes(640, 10, 256, 64, 10) == 0
    assert _beam(l, K=4097, n=64) == -2 and b"K <= 4096" in l.rqhip_last_error()
    assert _beam(l, K=256, n=65) == -2 and b"n_cands <= 64" in l.rqhip_last_error()
    assert _beam(l, h=1, beams_in=65, k=65, parents=True) == -2 and b"k <= 64" in l.rqhip_last_error()
    assert _beam(l, h=16, beams_in=10, H=16, parents=True) == -2 and b"RQHIP_MAX_PREFIX_LEN" in l.rqhip_last_error()
    assert _beam(l, K=32, n=40, k=10) == -1 and b"exceeds K" in l.rqhip_last_error()       # n_cands > K
    assert _beam(l, n=8, k=10) == -1 and b"candidates" in l.rqhip_last_error()             # k > beams_in * n
    assert _beam(l, h=0, beams_in=10) == -1                                                 # h = 0 takes one row per user
    assert _beam(l, h=3, beams_in=10, H=3, parents=True) == -1 and b"id levels" in l.rqhip_last_error()
    assert _beam(l, ld_logits=100) == -1 and b"ld_logits" in l.rqhip_last_error()
    assert _beam(l, N=5) == -1 and b"bad corpus" in l.rqhip_last_error()                   # null corpus
    assert _beam(l) == -1 and b"null pointer" in l.rqhip_last_error()                 # null logits
    assert _beam(l, h=1, beams_in=10) == -1                                            # null parents at h > 0
    assert _beam(l, B=0) == -3                                                         # no index
