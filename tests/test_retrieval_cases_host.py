"""tests/retrieval_cases.py on the host: every accuracy check of the retrieval model goes through `gate`, every switch of
an implementation through `impls` and every synthetic batch through `synthetic_batch`, so each is shown able to fail.
No GPU needed."""
import pytest
import torch

from retrieval_cases import gate, impls, synthetic_batch, tiny_model

U = 2.0 ** -22          # one fp32 ulp of 2
REF64 = torch.tensor([1.0, 2.0], dtype=torch.float64)
REF32 = torch.tensor([1.0, 2.0 + U])          # e_torch = 2^-23


def _got(ulps):
    return torch.tensor([1.0, 2.0 + ulps * U])


def test_gate_holds_the_kernel_to_factor_times_the_operators_error():
    gate("at the bound", _got(8), REF32, REF64, 8)
    for floor in ({}, {"floor": 0.0}):
        with pytest.raises(AssertionError, match="past the bound"):
            gate("past the bound", _got(9), REF32, REF64, 8, **floor)


def test_gate_floor_applies_where_the_operators_are_exact():
    exact = REF64.float()
    gate("one ulp", _got(1), exact, REF64, 8)                 # e_kernel = 2^-23 under the floor of 2^-22
    with pytest.raises(AssertionError, match="one ulp"):
        gate("one ulp", _got(1), exact, REF64, 8, floor=0.0)
    with pytest.raises(AssertionError, match="three ulps"):
        gate("three ulps", _got(3), exact, REF64, 8)          # e_kernel = 3 * 2^-23


def test_gate_demands_exact_zero_of_a_zero_reference():
    zero64 = torch.zeros(2, dtype=torch.float64)
    gate("zero", torch.zeros(2), torch.zeros(2), zero64, 8)
    with pytest.raises(AssertionError, match="tiny"):
        gate("tiny", torch.tensor([0.0, 1e-30]), torch.zeros(2), zero64, 8)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_gate_rejects_what_is_not_finite(bad):
    got = torch.tensor([1.0, bad])
    for ref32, ref64 in ((REF32, REF64), (REF64.float(), REF64), (torch.zeros(2), torch.zeros(2, dtype=torch.float64))):
        for floor in ({}, {"floor": 0.0}):
            with pytest.raises(AssertionError, match="not finite"):
                gate("not finite", got, ref32, ref64, 8, **floor)


def _choices(m):
    return [(x.attention_impl, x.norm_impl, x.ffn_impl) for x in (m, m.encoder.encoder, m.t5_decoder)] + [m.head_impl]


def test_impls_sets_all_four_on_both_stacks_and_restores_them():
    m = tiny_model().eval()
    with impls(m, attention="hip_train", norm="hip", ffn="hip", head="hip") as inside:
        assert inside is m and _choices(m) == [("hip_train", "hip", "hip")] * 3 + ["hip"]
        m.train()
    assert _choices(m) == [("torch", "torch", "torch")] * 3 + ["torch"] and not m.training
    with pytest.raises(RuntimeError, match="inside the block"):
        with impls(m, attention="hip", norm="hip", ffn="hip", head="hip"):
            m.bos_token.grad = torch.ones_like(m.bos_token)
            raise RuntimeError("inside the block")
    assert _choices(m) == [("torch", "torch", "torch")] * 3 + ["torch"] and m.bos_token.grad is None


# at 2 items "row1" and "b_mod_items" pad alike; at 3 items they do not
@pytest.mark.parametrize("pad,items,tails", [("none", 2, {}), ("row1", 2, {1: 1}), ("b_mod_items", 2, {1: 1}),
                                             ("row1", 3, {1: 1}), ("b_mod_items", 3, {1: 1, 2: 2})])
def test_synthetic_batch_shapes_padding_and_replay(pad, items, tails):
    B, L, K, N = 3, 3, 16, 50
    corpus = torch.randint(0, K, (N, L), generator=torch.Generator().manual_seed(4))
    batch = synthetic_batch(corpus, B, items, torch.Generator().manual_seed(5), pad=pad)
    assert [(t.shape, t.dtype) for t in batch[:4]] == [((B, 1), torch.int64), ((B, items * (L + 1)), torch.int64),
                                                       ((B, L + 1), torch.int64), ((B, items * (L + 1)), torch.bool)]
    assert batch[4] is None and batch[5] is None
    padded = torch.zeros(B, items, L + 1, dtype=torch.bool)
    for b, n in tails.items():
        padded[b, items - n:] = True
    padded = padded.reshape(B, -1)
    assert torch.equal(batch.seq_mask, ~padded) and torch.equal(batch.sem_ids == -1, padded)
    kept = batch.sem_ids.reshape(B, items, L + 1)[~padded.reshape(B, items, L + 1)[..., 0]]
    assert not bool(kept[:, L].any()) and not bool(batch.sem_ids_fut[:, L].any())          # the dedup column
    assert bool((kept[:, None, :L] == corpus[None]).all(-1).any(-1).all())                 # kept items are corpus rows
    assert bool(((batch.user_ids >= 0) & (batch.user_ids < 100)).all())
    again = synthetic_batch(corpus, B, items, torch.Generator().manual_seed(5), pad=pad)
    assert all(torch.equal(a, b) for a, b in zip(batch[:4], again[:4]))
    # without user ids: zeros, and the other tensors as before
    quiet = synthetic_batch(corpus, B, items, torch.Generator().manual_seed(5), pad=pad, user_ids=False)
    assert not bool(quiet.user_ids.any()) and all(torch.equal(a, b) for a, b in zip(batch[1:4], quiet[1:4]))
