"""proj_impl = "hip" on the T5 stacks and the retrieval model (modules/t5.py, modules/model.py): the attention projections
as grouped calls of csrc/t5_proj.hip, under every attention_impl and with the other fused forms on and off.

Losses and gradients: the small model of retrieval_cases (d_model 64, 2 heads, d_ff 96, 2 layers, K = 16, L = 3, batch 3;
encoder T = 9 with one padded row, decoder T = 4) against the same module in fp64 on the CPU.  Gates:
retrieval_cases.gate, e = max|a - a64| / max|a64| per tensor, e_kernel <= max(4 e_torch, 2^-22) for the loss, max(8
e_torch, 2^-22) for parameter gradients, e_torch from proj_impl = "torch" with the same other implementations on the same
device.

Generate: the recorded fixtures a, b, c with their recorded noise and attention_impl = "hip", proj_impl = "hip" against
proj_impl = "torch".  A user may be set aside only when its beams differ AND the operator run flags it within retrieval_cases.GAP of a
sampling boundary (another correct fp32 evaluation may then sample other codes); at most one per fixture.  The
log-probability tolerance is four times (the factor of the kernel gates) the distance the fp32 operator path itself
keeps from the same model in fp64 (retrieval_cases._cache_free_generate), measured by the test on the same fixture.
Measured: profiles/t5_proj_error.txt."""
import contextlib

import pytest
import torch

from conftest import load_golden
from retrieval_cases import (CASES, LAYERS, _cache_free_generate, _close, _Replay, build_model, compare_beams,
                             default_model_and_batch, fixture_batch, gate, impls, loss_and_grads, reference, same_bits,
                             small_model, tiny_batch, tiny_model, to_device)

pytestmark = pytest.mark.gpu

SMALL = (12, 96, False)         # retrieval_cases.small_model: seed, d_ff, norm weights as initialised


@contextlib.contextmanager
def proj(model, value="hip"):
    """proj_impl on `model` inside the block, "torch" again after it (the small model is shared by the test modules)."""
    model.proj_impl = value
    try:
        yield model
    finally:
        model.proj_impl = "torch"
        model._push_attention_impl()


def _count(monkeypatch, t5):
    calls = {"fwd": 0, "bwd": 0, "groups": []}
    o_f, o_b = t5.ops.t5_proj_fwd, t5.ops.t5_proj_bwd

    def fwd(x, weights, outs=None):
        calls["fwd"] += 1
        calls["groups"].append(len(weights))
        return o_f(x, weights, outs)

    def bwd(*a, **kw):
        calls["bwd"] += 1
        return o_b(*a, **kw)

    monkeypatch.setattr(t5.ops, "t5_proj_fwd", fwd)
    monkeypatch.setattr(t5.ops, "t5_proj_bwd", bwd)
    return calls


@pytest.mark.parametrize("others", ["torch", "hip"])
@pytest.mark.parametrize("attention", ["torch", "hip_train"])
def test_eval_loss_and_gradients_against_fp64(attention, others):
    model, _, batch, _ = small_model(*SMALL)
    loss64, grads64 = reference(*SMALL)
    kw = dict(attention=attention, norm=others, ffn=others, head=others)
    with impls(model.eval(), **kw):
        loss32, grads32 = loss_and_grads(model, batch)
    with impls(model, **kw), proj(model):
        loss, grads = loss_and_grads(model, batch)
    assert sorted(grads) == sorted(grads64) == sorted(grads32) and len(grads) > 40
    gate(f"{attention}/{others} loss", loss.reshape(1), loss32.reshape(1), loss64.reshape(1), 4)
    for n in sorted(grads):
        gate(f"{attention}/{others} grad {n}", grads[n], grads32[n], grads64[n], 8)


@pytest.mark.parametrize("attention", ["torch", "hip_train"])
def test_call_counts(attention, monkeypatch):
    import modules.t5 as t5
    model, _, batch, _ = small_model(*SMALL)
    calls = _count(monkeypatch, t5)
    # 2 per encoder block, 4 per decoder block, 1 for the cross-attention K/V of all blocks
    per_forward = 6 * LAYERS + 1
    groups = sorted([3, 1] * LAYERS + [3, 1, 1, 1] * LAYERS + [2 * LAYERS])
    with impls(model.eval(), attention=attention):
        loss_and_grads(model, batch)
        with torch.no_grad():
            model(batch)
        assert calls["fwd"] == 0 and calls["bwd"] == 0                # "torch": the grouped op is never called
        with proj(model):
            loss_and_grads(model, batch)
            assert (calls["fwd"], calls["bwd"]) == (per_forward, per_forward) and sorted(calls["groups"]) == groups
            calls.update(fwd=0, bwd=0, groups=[])
            with torch.no_grad():
                model(batch)
            assert (calls["fwd"], calls["bwd"]) == (per_forward, 0) and sorted(calls["groups"]) == groups
            calls.update(fwd=0, bwd=0, groups=[])
            model.train()                                              # train mode: the same calls
            loss_and_grads(model, batch, seed=3)
            assert (calls["fwd"], calls["bwd"]) == (per_forward, per_forward)


def test_unsupported_width_runs_the_operators_and_the_state_dict_is_the_same(monkeypatch):
    import modules.t5 as t5
    dev = torch.device("cuda")
    model = tiny_model().to(dev).eval()                 # d_model 8: no kernel for it
    batch = to_device(tiny_batch(), dev)
    keys = sorted(model.state_dict())
    calls = _count(monkeypatch, t5)
    want, want_g = loss_and_grads(model, batch)
    with torch.no_grad():
        want_n = model(batch).loss
    model.proj_impl = "hip"
    got, got_g = loss_and_grads(model, batch)
    with torch.no_grad():
        got_n = model(batch).loss
    assert calls["fwd"] == 0 and calls["bwd"] == 0
    assert same_bits(got, want) and same_bits(got_n, want_n) and sorted(got_g) == sorted(want_g) and len(got_g) > 10
    for n in want_g:
        assert same_bits(got_g[n], want_g[n]), n
    assert sorted(model.state_dict()) == keys
    small = small_model(*SMALL)[0]
    keys = sorted(small.state_dict())
    with proj(small):
        with torch.no_grad():
            small(small_model(*SMALL)[2])
        assert sorted(small.state_dict()) == keys


def _generate(model, batch, noise, monkeypatch, flag_boundaries=False):
    """One generate on the replayed noise -> (ids, log-probabilities, per user: whether at some step the n-th and the
    (n+1)-th sampling key of one of its rows lie within GAP)."""
    import modules.model as mm
    orig = mm.ops.beam_step
    tied = []

    def recording(logits, q, parent_scores, parent_ids, index, corpus, n, k):
        beams_in = 1 if parent_ids is None else parent_ids.shape[1]
        kv = torch.sort(torch.softmax(logits, dim=-1) / q, dim=-1, descending=True, stable=True).values
        if n < kv.shape[1]:
            tied.append((_close(kv[:, n - 1], kv[:, n]) & (kv[:, n - 1] > 0)).reshape(-1, beams_in).any(dim=1))
        return orig(logits, q, parent_scores, parent_ids, index, corpus, n, k)

    monkeypatch.setattr(mm, "_exponential_like", _Replay(noise))
    if flag_boundaries:
        monkeypatch.setattr(mm.ops, "beam_step", recording)
    try:
        out = model.generate_next_sem_id(batch)
    finally:
        monkeypatch.setattr(mm.ops, "beam_step", orig)
    boundary = torch.stack(tied).any(dim=0) if tied else torch.zeros(out.sem_ids.shape[0], dtype=torch.bool,
                                                                      device=out.sem_ids.device)
    return out.sem_ids, out.log_probas, boundary


def _operator_distance_to_fp64(fx, dev, noise, monkeypatch):
    """max |log-probability of the fp32 operator path - that of the same model in fp64| over the users whose beams the
    two runs agree on."""
    model = build_model(fx, dev).eval()
    batch = fixture_batch(fx, dev)
    ids32, lp32, _ = _generate(model, batch, noise, monkeypatch)
    ids64, lp64, _ = _cache_free_generate(model.double(), batch, [q.double() for q in noise])
    fin = torch.isfinite(lp64)
    same = ((torch.isfinite(lp32) == fin) & ((ids32 == ids64).all(dim=-1) | ~fin)).all(dim=1)
    assert int(same.sum()) >= same.numel() - 2, "the fp32 operators and fp64 disagree on too many users to measure"
    use = fin & same.unsqueeze(1)
    return float((lp32.double() - lp64)[use].abs().max())


@pytest.mark.parametrize("case", CASES)
def test_generate_matches_the_operator_projections_on_recorded_noise(case, monkeypatch):
    fx = load_golden(f"retrieval_{case}.npz")
    dev = torch.device("cuda")
    L = int(fx["config"][0])
    noise = [torch.from_numpy(fx[f"noise{h}"]).to(dev) for h in range(L)]
    d_op = _operator_distance_to_fp64(fx, dev, noise, monkeypatch)
    tol = 4 * d_op
    model = build_model(fx, dev).eval()
    batch = fixture_batch(fx, dev)
    model.attention_impl = "hip"
    r_ids, r_lp, boundary = _generate(model, batch, noise, monkeypatch, flag_boundaries=True)
    import modules.t5 as t5
    calls = _count(monkeypatch, t5)
    model.proj_impl = "hip"
    ids, lp, _ = _generate(model, batch, noise, monkeypatch)
    # fixture b has d_model 24, which no kernel takes: there the operators run and the comparison is one of equal bits
    assert (calls["fwd"] > 0) == (int(fx["config"][2]) % 32 == 0) and calls["bwd"] == 0
    fin = torch.isfinite(r_lp)
    dlp = torch.where(fin & torch.isfinite(lp), (lp - r_lp).abs(), torch.zeros_like(r_lp))
    differs = ((torch.isfinite(lp) != fin) | (dlp > tol) | (fin & (ids != r_ids).any(dim=-1))).any(dim=1)
    print(f"fixture {case}: fp32 operators to fp64 {d_op:.3e}, tolerance {tol:.3e}, max |log_proba(hip) - log_proba(torch)| "
          f"{float(dlp.max()):.3e} (of the users kept: {float(dlp[~differs].max()) if bool((~differs).any()) else 0.0:.3e}), "
          f"{int(differs.sum())} of {differs.numel()} users differ, {int(boundary.sum())} flagged on a sampling boundary")
    # a user that differs sits on a sampling boundary of the operator-projection run, and only such a user is set aside
    assert bool(boundary[differs].all()), "a user differs away from a sampling boundary"
    assert int(differs.sum()) <= 1
    keep = ~differs
    amb = (_close(r_lp[:, :-1], r_lp[:, 1:]) & torch.isfinite(r_lp[:, :-1])).any(dim=1)
    compare_beams(ids[keep], lp[keep], None, r_ids[keep], r_lp[keep], None, amb[keep], tol)


def test_decode_steps_write_the_slabs_and_attention_reads_them(monkeypatch):
    """Each decode step's grouped call leaves in the slab position the bits of a separate one-weight call for k and
    for v; no torch.mm runs; the K/V pointers that reach ops.t5_attention are the slabs' own."""
    import modules.t5 as t5
    dev = torch.device("cuda")
    model, batch = default_model_and_batch(dev, B=16, N=3000, seed=2)
    model.attention_impl, model.proj_impl = "hip", "hip"
    slab_calls, kv_ptrs, caches, mms = [], [], [], []
    o_proj, o_att, o_cache, o_mm = t5.ops.t5_proj_fwd, t5.ops.t5_attention, t5.T5Stack.new_decode_cache, torch.mm

    def spy_proj(x, weights, outs=None):
        res = o_proj(x, weights, outs)
        if outs is not None:
            assert len(weights) == 3 and outs[0] is None and res[1] is outs[1] and res[2] is outs[2]
            for j in (1, 2):
                alone = o_proj(x, [weights[j]])[0]
                assert same_bits(outs[j], alone.view(outs[j].shape)), j
            slab_calls.append((outs[1].data_ptr(), outs[2].data_ptr(), outs[1].shape[0]))
        return res

    def spy_att(q, k, v, *a, **kw):
        kv_ptrs.append((k.data_ptr(), v.data_ptr(), kw.get("anc") is not None))
        return o_att(q, k, v, *a, **kw)

    def spy_cache(self, *a, **kw):
        caches.append(o_cache(self, *a, **kw))
        return caches[-1]

    def spy_mm(*a, **kw):
        mms.append(1)
        return o_mm(*a, **kw)

    monkeypatch.setattr(t5.ops, "t5_proj_fwd", spy_proj)
    monkeypatch.setattr(t5.ops, "t5_attention", spy_att)
    monkeypatch.setattr(t5.T5Stack, "new_decode_cache", spy_cache)
    monkeypatch.setattr(torch, "mm", spy_mm)
    torch.manual_seed(4)
    model.generate_next_sem_id(batch)
    L, blocks, k = model.num_hierarchies, len(model.t5_decoder.block), model.top_k_for_generation
    B = batch.sem_ids.shape[0]
    assert not mms and len(caches) == 1 and len(slab_calls) == L * blocks
    slabs = caches[0].slabs
    inner = slabs[0][0].shape[-1]
    for c, (kp, vp, rows) in enumerate(slab_calls):
        h, i = divmod(c, blocks)
        assert rows == (B if h == 0 else B * k)
        assert kp == slabs[i][0].data_ptr() + 4 * h * B * k * inner and vp == slabs[i][1].data_ptr() + 4 * h * B * k * inner
    slab_ptrs = {(ks.data_ptr(), vs.data_ptr()) for ks, vs in slabs}
    cached = [(kp, vp) for kp, vp, has_anc in kv_ptrs if has_anc]
    assert len(cached) == L * blocks and all(p in slab_ptrs for p in cached)


def test_generate_under_graph_capture_equals_eager(monkeypatch):
    import modules.model as mm
    dev = torch.device("cuda")
    model, batch = default_model_and_batch(dev, B=16, N=3000, seed=3)
    model.attention_impl, model.proj_impl = "hip", "hip"
    L, K, k = model.num_hierarchies, model.num_embeddings_per_hierarchy, model.top_k_for_generation
    B = batch.sem_ids.shape[0]
    torch.manual_seed(11)
    noise = [torch.empty(B * (1 if h == 0 else k), K, device=dev).exponential_(1) for h in range(L)]

    class Static:
        def __init__(self):
            self.i = 0

        def __call__(self, p):
            q = noise[self.i % L]
            self.i += 1
            return q

    monkeypatch.setattr(mm, "_exponential_like", Static())
    eager = model.generate_next_sem_id(batch)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            model.generate_next_sem_id(batch)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = model.generate_next_sem_id(batch)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured.sem_ids, eager.sem_ids)
    assert same_bits(captured.log_probas, eager.log_probas)
    assert torch.isfinite(eager.log_probas).any()
