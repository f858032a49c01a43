"""head_impl = "hip" on the retrieval model (modules/model.py): the heads and their cross-entropy losses of `forward` as
one autograd.SidHeadLossFunction call (csrc/sid_head_loss.hip).

The small model, batch, fp64 reference and gates of tests/test_gpu_t5_norm_impl.py (d_model 64, 2 heads, d_ff 128, 2
layers, K = 16, L = 3, batch 3): e = max|a - a64| / max|a64| per tensor, e_kernel <= max(4 e_torch, 2^-22) for the loss
and max(8 e_torch, 2^-22) for every parameter gradient (retrieval_cases.gate), e_torch from head_impl = "torch" with the
same attention_impl and norm_impl on the same device."""
import pytest
import torch

from retrieval_cases import gate, impls, loss_and_grads, reference, same_bits, small_model

pytestmark = pytest.mark.gpu

SMALL = (11, 128, True)         # the set-up of tests/test_gpu_t5_norm_impl.py
PAIRS = [("torch", "torch"), ("hip_train", "hip")]


def _count(monkeypatch):
    import modules.model as mm
    calls = {"fwd": 0, "bwd": 0}
    o_f, o_b = mm.ops.sid_head_loss_fwd, mm.ops.sid_head_loss_bwd

    def fwd(*a, **kw):
        calls["fwd"] += 1
        return o_f(*a, **kw)

    def bwd(*a, **kw):
        calls["bwd"] += 1
        return o_b(*a, **kw)

    monkeypatch.setattr(mm.ops, "sid_head_loss_fwd", fwd)
    monkeypatch.setattr(mm.ops, "sid_head_loss_bwd", bwd)
    return calls


@pytest.fixture
def model():
    return small_model(*SMALL)[0].eval()


@pytest.mark.parametrize("attention,norm", PAIRS)
def test_eval_loss_and_gradients_against_fp64(model, attention, norm):
    batch = small_model(*SMALL)[2]
    loss64, grads64 = reference(*SMALL)
    with impls(model, attention=attention, norm=norm):
        loss32, grads32 = loss_and_grads(model, batch)
    with impls(model, attention=attention, norm=norm, head="hip"):
        loss, grads = loss_and_grads(model, batch)
    assert sorted(grads) == sorted(grads64) == sorted(grads32) and len(grads) > 40
    gate(f"{attention}/{norm} loss", loss.reshape(1), loss32.reshape(1), loss64.reshape(1), 4)
    for n in sorted(grads):
        gate(f"{attention}/{norm} grad {n}", grads[n], grads32[n], grads64[n], 8)


@pytest.mark.parametrize("attention,norm", PAIRS)
def test_output_shape_and_call_counts(model, attention, norm, monkeypatch):
    batch = small_model(*SMALL)[2]
    calls = _count(monkeypatch)
    with impls(model, attention=attention, norm=norm):
        loss_and_grads(model, batch)
        with torch.no_grad():
            model(batch)
        assert calls == {"fwd": 0, "bwd": 0}                    # "torch": the fused op is never called
    with impls(model, attention=attention, norm=norm, head="hip"):
        out = model(batch)
        assert calls == {"fwd": 1, "bwd": 0}
        assert out.logits is None and out.loss.shape == () and out.loss.dtype == torch.float32 and out.loss.requires_grad
        assert out.loss_d.shape == (3,) and not out.loss_d.requires_grad
        total = torch.zeros((), device=out.loss.device)
        for h in range(3):
            total = total + out.loss_d[h]
        assert same_bits(total, out.loss.detach())
        out.loss.backward()
        assert calls == {"fwd": 1, "bwd": 1}
        with torch.no_grad():
            quiet = model(batch)
        assert calls == {"fwd": 2, "bwd": 1}
        assert not quiet.loss.requires_grad and same_bits(quiet.loss, out.loss.detach())
        assert same_bits(quiet.loss_d, out.loss_d)


def test_train_mode_replays_under_a_seed(model):
    batch = small_model(*SMALL)[2]
    with impls(model, attention="hip_train", norm="hip", head="hip"):
        model.train()
        loss_a, grads_a = loss_and_grads(model, batch, seed=5)
        loss_b, grads_b = loss_and_grads(model, batch, seed=5)
    assert torch.isfinite(loss_a) and same_bits(loss_a, loss_b)
    assert sorted(grads_a) == sorted(grads_b) and len(grads_a) > 40
    for n in grads_a:
        assert same_bits(grads_a[n], grads_b[n]), n


def test_unsupported_width_runs_the_operators(monkeypatch):
    from modules.model import EncoderDecoderRetrievalModel
    batch = small_model(*SMALL)[2]
    torch.manual_seed(2)
    m = EncoderDecoderRetrievalModel(torch.zeros(4, 3, dtype=torch.long), 3, 16, t5_d_model=66, t5_num_heads=1, t5_d_ff=32,
                                     t5_num_layers=1).to(torch.device("cuda")).eval()
    calls = _count(monkeypatch)
    want, want_g = loss_and_grads(m, batch)
    m.head_impl = "hip"
    got, got_g = loss_and_grads(m, batch)
    assert calls == {"fwd": 0, "bwd": 0} and torch.equal(got, want) and sorted(got_g) == sorted(want_g)
    for n in want_g:
        assert torch.equal(got_g[n], want_g[n]), n


def test_generate_is_untouched(model):
    batch = small_model(*SMALL)[2]
    torch.manual_seed(1)
    want = model.generate_next_sem_id(batch)
    with impls(model, head="hip"):
        torch.manual_seed(1)
        got = model.generate_next_sem_id(batch)
    assert torch.equal(got.sem_ids, want.sem_ids) and same_bits(got.log_probas, want.log_probas)
