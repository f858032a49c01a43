"""The retrieval model on the GPU: ops.beam_step (csrc/beam_step.hip) against the reference's operator sequence,
torch.multinomial's exponential race on the device, forward / gradients / generate against the reference's recorded
values (tests/golden/retrieval_*.npz), self-consistency at the default config and a training smoke test."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from retrieval_cases import (CASES, GAP, _cache_free_generate, _close, _corpus, _Replay, build_model, check_forward, compare_beams,
                             default_model_and_batch, fixture_batch, ref_beam_step, same_bits)

pytestmark = pytest.mark.gpu

# the step's domain: n <= K, and k <= n at the first step (one row per user)
STEP_SHAPES = [(K, n, k, h) for K in (8, 256, 4096) for n in (8, 64) for k in (1, 10, 64) for h in (0, 1, 2)
               if n <= K and (h > 0 or k <= n)]


@pytest.mark.parametrize("K,n,k,h", STEP_SHAPES)
def test_beam_step_matches_reference_ops(K, n, k, h):
    from rqhip import ops
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(K * 7 + n * 3 + k + h)
    L, B = 3, 24
    corpus = _corpus(K, L, 3000, g, dev)
    index = ops.prefix_index_build(corpus)
    beams_in = 1 if h == 0 else k
    rows = B * beams_in
    logits = (torch.randn(rows, K, generator=g) * 3.0).to(dev)
    logits[::5] *= 200.0                        # softmax underflows to exact zeros in these rows
    torch.manual_seed(K + n + k + h)
    noise = torch.empty(rows, K, device=dev).exponential_(1)
    if h:
        pick = torch.randint(0, corpus.shape[0], (B, beams_in), generator=g).to(dev)
        parent_ids = corpus[pick][:, :, :h].contiguous()
        parent_ids[:, ::3, -1] = torch.randint(0, K, (B, (beams_in + 2) // 3), generator=g).to(dev)
        parent_scores = -torch.rand(B, beams_in, generator=g).to(dev) * 5.0
        parent_scores[::4, -1] = float("-inf")
        parent_scores = parent_scores.sort(dim=1, descending=True).values.contiguous()
    else:
        parent_ids = parent_scores = None
    ids, scores, parent = ops.beam_step(logits, noise, parent_scores, parent_ids, index, corpus, n, k)
    r_ids, r_scores, r_parent, amb = ref_beam_step(logits, noise, parent_scores, parent_ids, index, corpus, n, k)
    assert ids.shape == (B, k, h + 1) and scores.shape == (B, k) and parent.shape == (B, k)
    n_amb = compare_beams(ids, scores, parent, r_ids, r_scores, r_parent, amb, 2e-6)
    print(f"K={K} n={n} k={k} h={h}: {n_amb}/{B} users decided inside the {GAP:g} gap, "
          f"{int((~torch.isfinite(r_scores)).sum())} -inf beams")
    assert n_amb <= B // 4
    # deterministic
    again = ops.beam_step(logits, noise, parent_scores, parent_ids, index, corpus, n, k)
    assert torch.equal(again[0], ids) and same_bits(again[1], scores)


@pytest.mark.parametrize("K,n", [(16, 16), (256, 64), (4096, 64)])
def test_multinomial_is_the_exponential_race_on_device(K, n):
    dev = torch.device("cuda")
    p = F.softmax(torch.randn(97, K, device=dev) * 2.0, dim=-1)
    torch.manual_seed(1234)
    a = torch.multinomial(p, n)
    torch.manual_seed(1234)
    q = torch.empty_like(p).exponential_(1)
    b = torch.topk(p / q, n).indices
    assert torch.equal(a, b)


@pytest.mark.parametrize("case", CASES)
def test_forward_and_gradients_match_reference_gpu(case):
    fx = load_golden(f"retrieval_{case}.npz")
    dev = torch.device("cuda")
    check_forward(fx, build_model(fx, dev), fixture_batch(fx, dev))


@pytest.mark.parametrize("case", CASES)
def test_generate_matches_reference_with_recorded_noise(case, monkeypatch):
    import modules.model as mm
    fx = load_golden(f"retrieval_{case}.npz")
    dev = torch.device("cuda")
    model = build_model(fx, dev).eval()
    L = int(fx["config"][0])
    monkeypatch.setattr(mm, "_exponential_like", _Replay([torch.from_numpy(fx[f"noise{h}"]).to(dev) for h in range(L)]))
    out = model.generate_next_sem_id(fixture_batch(fx, dev))
    r_ids = torch.from_numpy(fx["sem_ids"]).to(dev)
    r_lp = torch.from_numpy(fx["log_probas"]).to(dev)
    ss = r_lp
    amb = (_close(ss[:, :-1], ss[:, 1:]) & torch.isfinite(ss[:, :-1])).any(dim=1)
    n_amb = compare_beams(out.sem_ids, out.log_probas, None, r_ids, r_lp, None, amb, 1e-5)
    print(f"fixture {case}: {n_amb} users inside the gap")
    assert n_amb == 0


def test_generate_self_consistency_default_config(monkeypatch):
    import modules.model as mm
    from evaluate.metrics import TopKAccumulator
    from rqhip import ops
    dev = torch.device("cuda")
    model, batch = default_model_and_batch(dev)
    L, k = model.num_hierarchies, model.top_k_for_generation
    B = batch.sem_ids.shape[0]
    # record the noise the model draws
    drawn = []
    orig = mm._exponential_like

    def record(p):
        q = orig(p)
        drawn.append(q.clone())
        return q

    monkeypatch.setattr(mm, "_exponential_like", record)
    torch.manual_seed(7)
    out = model.generate_next_sem_id(batch)
    monkeypatch.setattr(mm, "_exponential_like", orig)
    assert out.sem_ids.shape == (B, k, L) and out.log_probas.shape == (B, k)
    r_ids, r_lp, amb = _cache_free_generate(model, batch, drawn)
    n_amb = compare_beams(out.sem_ids, out.log_probas, None, r_ids, r_lp, None, amb, 1e-5, 1e-5)
    print(f"default config: {n_amb}/{B} users inside the gap, {int(torch.isfinite(r_lp).sum())} finite beams")
    assert n_amb <= B // 8
    fin = torch.isfinite(out.log_probas)
    assert fin.any()
    # the finite beams are corpus items
    valid = ops.prefix_lookup(model._prefix_index._index, model._prefix_index._corpus, out.sem_ids.reshape(-1, L))
    assert bool(valid.reshape(B, k)[fin].all())
    # the metrics consume the output
    acc = TopKAccumulator(ks=[1, 5, 10])
    acc.accumulate(actual=batch.sem_ids_fut[:, :L], top_k=out.sem_ids)
    res = acc.reduce()
    assert set(res) >= {"ndcg", "h@1", "h@5", "h@10"} and all(np.isfinite(v) for v in res.values())
    # a seeded generate replays bit for bit
    torch.manual_seed(7)
    again = model.generate_next_sem_id(batch)
    assert torch.equal(again.sem_ids, out.sem_ids)
    assert same_bits(again.log_probas, out.log_probas)


def test_generate_under_graph_capture_equals_eager(monkeypatch):
    import modules.model as mm
    dev = torch.device("cuda")
    model, batch = default_model_and_batch(dev, B=32, N=5000, seed=3)
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


def test_training_smoke_amazon_shape():
    dev = torch.device("cuda")
    from modules.model import EncoderDecoderRetrievalModel
    model, batch = default_model_and_batch(dev, B=64, N=12101, d=128, seed=5)
    torch.manual_seed(5)
    model = EncoderDecoderRetrievalModel(model.codebooks, 3, 256, t5_d_model=384, t5_num_heads=6, t5_d_ff=1024,
                                         t5_num_layers=4).to(dev)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    model.train()
    losses = []
    for _ in range(3):
        opt.zero_grad()
        out = model(batch)
        out.loss.backward()
        opt.step()
        losses.append(out.loss.item())
        assert all(torch.isfinite(p).all() for p in model.parameters())
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
