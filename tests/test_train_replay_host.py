"""The mask log and its replay (tests/retrieval_cases.py: recording, replaying, record_step, replay_step) on the host,
with the operator model only: what tests/test_gpu_train_replay.py relies on is shown able to fail.  No GPU needed.

The model is retrieval_cases.small_model(12, 96, True) on the CPU: d_model 64, 2 heads, d_ff 96, 2 layers, batch 3,
dropout rate 0.1.  A stack forward has 2 + 4 * layers sites in the encoder and 2 + 6 * layers in the decoder."""
import copy

import pytest
import torch

from retrieval_cases import (FLOOR, LAYERS, MaskLog, SiteMismatch, err, loss_and_grads, record_step, recording,
                             replay_step, replaying, same_bits, small_model)

SMALL = (12, 96, True, "cpu")
SITES = (2 + 4 * LAYERS) + (2 + 6 * LAYERS)


def _models():
    model, model64, batch, _ = small_model(*SMALL)
    return model, model64, batch


def _same(a, b):
    (loss_a, grads_a), (loss_b, grads_b) = a, b
    assert same_bits(loss_a.reshape(1).float(), loss_b.reshape(1).float()) and torch.equal(loss_a, loss_b)
    assert sorted(grads_a) == sorted(grads_b) and len(grads_a) > 40
    for n in grads_a:
        assert torch.equal(grads_a[n], grads_b[n]), n


def _other_mask(site, seed):
    return torch.rand(site.keep.shape, generator=torch.Generator().manual_seed(seed)) >= site.p


def test_sites_come_in_the_order_of_the_stack_forward():
    model, _, batch = _models()
    *_, log = record_step(model, batch)
    B, d, H, F = 3, 64, 2, 96
    Te, Td = batch.sem_ids.shape[1], 4              # 4 columns per item: 3 ids and the separator
    enc = [(B, Te, d)] + [(B, H, Te, Te), (B, Te, d), (B, Te, F), (B, Te, d)] * LAYERS + [(B, Te, d)]
    dec = [(B, Td, d)] + [(B, H, Td, Td), (B, Td, d), (B, H, Td, Te), (B, Td, d), (B, Td, F), (B, Td, d)] * LAYERS + [
        (B, Td, d)]
    assert [tuple(s.keep.shape) for s in log.sites] == enc + dec and len(log) == SITES
    assert all(s.kind == "operator" and s.p == 0.1 and s.seed is None and s.keep.dtype == torch.bool for s in log.sites)
    assert not log.calls and not model.training


@pytest.mark.parametrize("double", [False, True])
def test_replaying_a_recorded_operator_step_gives_the_same_bits(double):
    model, model64, batch = _models()
    m = model64 if double else model
    loss, grads, log = record_step(m, batch, draw_seed=3)
    assert loss.dtype == (torch.float64 if double else torch.float32) and len(log) == SITES
    _same((loss, grads), replay_step(m, batch, log))
    _same((loss, grads), replay_step(m, batch, log))                 # a replay leaves the log as it was
    other = record_step(m, batch, draw_seed=4)
    assert not torch.equal(other[0], loss)                           # the masks decide the loss


def _without_dropout(model):
    from modules.t5 import T5Attention
    model = copy.deepcopy(model)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, T5Attention):
            m.dropout = 0.0
    model.encoder.encoder.config.dropout_rate = model.t5_decoder.config.dropout_rate = 0.0
    return model


@pytest.mark.parametrize("how", ["eval", "rate 0"])
def test_without_dropout_the_log_is_empty_and_the_replay_is_the_plain_run(how):
    model, _, batch = _models()
    model = _without_dropout(model).train() if how == "rate 0" else model
    assert model.training == (how == "rate 0")
    plain = loss_and_grads(model, batch)
    with recording() as log:
        recorded = loss_and_grads(model, batch)
    assert len(log) == 0 and not log.calls
    with replaying(log):
        replayed = loss_and_grads(model, batch)
    _same(plain, recorded)
    _same(plain, replayed)
    model.zero_grad(set_to_none=True)


def test_a_removed_site_and_a_wrong_shape_are_site_mismatches():
    model, _, batch = _models()
    *_, log = record_step(model, batch)
    # the first site's neighbour has another shape; the encoder's final p_in and p_out (sites 8 and 9) share one, so
    # without site 8 the log is one off until the decoder's embeddings; without the last site the log ends early
    for i, where in ((0, 0), (2 + 4 * LAYERS - 2, 2 + 4 * LAYERS - 1), (SITES - 1, SITES - 1)):
        with pytest.raises(SiteMismatch, match=rf"site {where}: the model drops a tensor of shape \(3, "):
            replay_step(model, batch, log.without(i))
    sites = list(log.sites)
    sites[4] = sites[4]._replace(keep=sites[4].keep[..., :-1])
    with pytest.raises(SiteMismatch, match=r"site 4: .* shape \(3, 8, 64\) .* shape \(3, 8, 63\)"):
        replay_step(model, batch, MaskLog(sites))
    sites = list(log.sites)
    sites[5] = sites[5]._replace(p=0.2)
    with pytest.raises(SiteMismatch, match=r"site 5: .* at p = 0.1, the log holds .* at p = 0.2"):
        replay_step(model, batch, MaskLog(sites))
    with pytest.raises(SiteMismatch, match=rf"site {SITES}: the log's operator mask of shape \(3, 4, 64\) .* 0 sites behind"):
        replay_step(model, batch, MaskLog(log.sites + [log.sites[-1]]))
    assert not model.training and all(p.grad is None for p in model.parameters())


@pytest.mark.parametrize("i", [0, 1, 3, 2 + 4 * LAYERS, SITES - 3, SITES - 1])
def test_one_mask_of_another_seed_is_no_rounding_noise(i):
    """Site i (the encoder's embeddings, an attention's weights, a feed-forward's inner activation, the decoder's
    embeddings, its last feed-forward, the final norm's output) with the mask of another seed: the fp64 loss and every
    parameter gradient -- all of them lie behind every site, forward or backward -- move by more than the bound the
    GPU gate allows a fused step, which is 4 (loss) or 8 (gradients) times the operators' own fp32 error, or FLOOR."""
    model, model64, batch = _models()
    _, _, log = record_step(model64, batch, draw_seed=7)
    loss64, grads64 = replay_step(model64, batch, log)
    loss32, grads32 = replay_step(model, batch, log)
    wrong = log.swapped(i, _other_mask(log.sites[i], 8))
    assert not torch.equal(wrong.sites[i].keep, log.sites[i].keep)
    loss_w, grads_w = replay_step(model64, batch, wrong)
    assert sorted(grads_w) == sorted(grads64) == sorted(grads32)
    assert err(loss_w.reshape(1), loss64.reshape(1)) > max(4 * err(loss32.reshape(1), loss64.reshape(1)), FLOOR)
    for n in grads64:
        assert err(grads_w[n], grads64[n]) > max(8 * err(grads32[n], grads64[n]), FLOOR), n
