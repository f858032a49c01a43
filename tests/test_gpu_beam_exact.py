"""The exact constrained beam search on the GPU (model.beam_impl = "exact"): ops.beam_topk_step
(csrc/beam_step.hip, rqhip_beam_topk_step) against the operators in fp64, `generate` against an exhaustive ranking of
a small corpus and against a cache-free restatement at the default config, and what "no random numbers" means: equal
bits under different seeds, an untouched generator, no noise draw, and a graph replay that equals eager.

Ambiguity.  The kernel scores in fp32, the references in fp64, so two candidates whose reference scores nearly agree
may legitimately come out in the other order.  A user is ambiguous when two neighbours among its first k + 1 reference
scores, the upper one finite, differ by at most GAP * max(1, |a|, |b|).  Everywhere else ids and parents are compared at
ALL k positions, the -inf ones included (equal scores go to the lower candidate number, so they are determined too)."""
import copy
import functools

import pytest
import torch

from retrieval_cases import (FLOOR, GAP, _corpus, compare_beams, default_model_and_batch, gate, same_bits, synthetic_batch,
                             to_device)

pytestmark = pytest.mark.gpu

# K: a wave wider than the row (8), a ragged last pass (100), the default (256), the LDS maximum (4096); k: 1, the
# default, the maximum; K = 8 with k = 64 keeps m = min(k, K) < k per row; K = 4096, k = 1, h = 2 has users without any
# valid candidate.  h = 0 takes one row per user, so k <= K there.
STEP_SHAPES = [(K, k, h) for K in (8, 100, 256, 4096) for k in (1, 10, 64) for h in (0, 1, 2) if h > 0 or k <= K]


def _near(a, b):
    """Neighbouring reference scores a >= b that fp32 may order the other way: a finite, |a - b| within the gap."""
    scale = torch.maximum(torch.maximum(a.abs(), b.abs()), torch.ones_like(a))
    return torch.isfinite(a) & torch.isfinite(b) & ((a - b).abs() <= GAP * scale)


def ref_topk_step(logits, parent_scores, parent_ids, index, corpus, k):
    """The exact step as operators in fp64: log_softmax plus the parent's score, -inf where ops.prefix_lookup says the
    prefix is not in the corpus, a stable descending sort of the [B, beams_in * K] row.  Returns ids, scores (fp64),
    parent, the kept candidates' numbers beam * K + code, and the ambiguous users."""
    from rqhip import ops
    rows, K = logits.shape
    beams_in = 1 if parent_ids is None else parent_ids.shape[1]
    h = 0 if parent_ids is None else parent_ids.shape[2]
    B = rows // beams_in
    dev = logits.device
    scores = torch.log_softmax(logits.double(), dim=-1).reshape(B, beams_in * K)
    codes = torch.arange(K, device=dev).repeat(beams_in).expand(B, -1).unsqueeze(-1)      # [B, beams_in * K, 1]
    if h:
        scores = scores + parent_scores.double().repeat_interleave(K, dim=1)
        prefix = torch.cat([parent_ids.repeat_interleave(K, dim=1), codes], dim=-1)
    else:
        prefix = codes
    valid = ops.prefix_lookup(index, corpus, prefix.reshape(-1, h + 1).contiguous()).reshape(B, -1)
    scores = scores.masked_fill(~valid, float("-inf"))
    sv, idx = torch.sort(scores, dim=-1, descending=True, stable=True)
    top = idx[:, :k]
    ids = torch.gather(prefix, 1, top.unsqueeze(-1).expand(-1, -1, h + 1))
    parent = top // K + torch.arange(B, device=dev).unsqueeze(1) * beams_in
    ss = sv[:, : min(k + 1, sv.shape[1])]
    amb = _near(ss[:, :-1], ss[:, 1:]).any(dim=1)
    return ids, sv[:, :k], parent, top, amb


def _step_inputs(K, k, h, dev):
    """The inputs of test_gpu_retrieval.py:test_beam_step_matches_reference_ops, without the noise."""
    from rqhip import ops
    g = torch.Generator().manual_seed(K * 7 + k * 3 + h)
    L, B = 3, 24
    corpus = _corpus(K, L, 3000, g, dev)
    index = ops.prefix_index_build(corpus)
    beams_in = 1 if h == 0 else k
    rows = B * beams_in
    logits = (torch.randn(rows, K, generator=g) * 3.0).to(dev)
    logits[::5] *= 200.0
    if h:
        pick = torch.randint(0, corpus.shape[0], (B, beams_in), generator=g).to(dev)
        parent_ids = corpus[pick][:, :, :h].contiguous()
        parent_ids[:, ::3, -1] = torch.randint(0, K, (B, (beams_in + 2) // 3), generator=g).to(dev)
        parent_scores = -torch.rand(B, beams_in, generator=g).to(dev) * 5.0
        parent_scores[::4, -1] = float("-inf")
        parent_scores = parent_scores.sort(dim=1, descending=True).values.contiguous()
    else:
        parent_ids = parent_scores = None
    return B, beams_in, corpus, index, logits, parent_scores, parent_ids


@pytest.mark.parametrize("K,k,h", STEP_SHAPES)
def test_beam_topk_step_matches_fp64_operators(K, k, h):
    from rqhip import ops
    dev = torch.device("cuda")
    B, beams_in, corpus, index, logits, parent_scores, parent_ids = _step_inputs(K, k, h, dev)
    ids, scores, parent = ops.beam_topk_step(logits, parent_scores, parent_ids, index, corpus, k)
    assert ids.shape == (B, k, h + 1) and scores.shape == (B, k) and parent.shape == (B, k)
    assert ids.dtype == torch.int64 and scores.dtype == torch.float32 and parent.dtype == torch.int64
    r_ids, r_scores, r_parent, top, amb = ref_topk_step(logits, parent_scores, parent_ids, index, corpus, k)
    fin = torch.isfinite(r_scores)
    n_amb = int(amb.sum())
    print(f"K={K} k={k} h={h}: {n_amb}/{B} users decided inside the {GAP:g} gap, {int((~fin).sum())} -inf beams, "
          f"{int((~fin).all(dim=1).sum())} users without a valid candidate")
    # the reference alone flags at most 4 of these 24 users at any shape: the cap hides no failure
    assert n_amb <= B // 4
    assert torch.equal(torch.isfinite(scores), fin), "-inf beams differ"
    assert not torch.isnan(scores).any() and bool((scores[~fin] == float("-inf")).all())
    ok = ~amb
    assert torch.equal(ids[ok], r_ids[ok]), "ids differ"
    assert torch.equal(parent[ok], r_parent[ok]), "parents differ"
    # scores of the finite beams: the operators in fp32 on the device are the yardstick, beams from a row of * 200
    # logits apart from the others so that their magnitude does not set the scale for the small ones
    ref32 = torch.log_softmax(logits, dim=-1).reshape(B, beams_in * K)
    if h:
        ref32 = ref32 + parent_scores.repeat_interleave(K, dim=1)
    ref32 = torch.gather(ref32, 1, top)
    big = (r_parent % 5) == 0
    for what, sel in (("x200 rows", big), ("other rows", ~big)):
        sel = sel & fin & ok.unsqueeze(1)
        gate(f"K={K} k={k} h={h} scores, {what}", scores[sel], ref32[sel], r_scores[sel], 4, FLOOR)
    # the same bits on a second call, and on logits with a row stride
    again = ops.beam_topk_step(logits, parent_scores, parent_ids, index, corpus, k)
    assert torch.equal(again[0], ids) and same_bits(again[1], scores) and torch.equal(again[2], parent)
    wide = torch.full((logits.shape[0], K + 8), float("nan"), device=dev)
    wide[:, :K] = logits
    strided = ops.beam_topk_step(wide[:, :K], parent_scores, parent_ids, index, corpus, k)
    assert torch.equal(strided[0], ids) and same_bits(strided[1], scores) and torch.equal(strided[2], parent)


def test_finite_beams_never_decrease_from_level_to_level():
    """Every kept finite beam is a corpus prefix and so has a valid child: the number of finite beams of a user can only
    grow until it reaches k.  Steps fed by hand, B = 8, the default K and k, on the default corpus (every first code
    occurs: k finite beams from the start) and on a sparse one (4 first codes, so the count has to grow)."""
    from rqhip import ops
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(5)
    B, K, k, L = 8, 256, 10, 3
    sparse = torch.stack([torch.tensor([3, 7, 100, 255])[torch.randint(0, 4, (40,), generator=g)],
                          torch.randint(0, 3, (40,), generator=g) * 100, torch.randint(0, K, (40,), generator=g)], dim=1)
    for name, corpus in (("default", _corpus(K, L, 20000, g, dev)), ("sparse", sparse.to(dev))):
        index = ops.prefix_index_build(corpus)
        ids = scores = None
        counts = []
        for h in range(L):
            logits = (torch.randn(B * (1 if h == 0 else k), K, generator=g) * 4.0).to(dev)
            ids, scores, parent = ops.beam_topk_step(logits, scores, ids, index, corpus, k)
            fin = torch.isfinite(scores)
            counts.append(fin.sum(dim=1))
            valid = ops.prefix_lookup(index, corpus, ids.reshape(-1, h + 1)).reshape(B, k)
            assert torch.equal(valid, fin)           # finite <=> a corpus prefix: the children of a -inf beam are none
            assert bool((scores[:, :-1] >= scores[:, 1:]).all())
            users = torch.arange(B, device=dev).unsqueeze(1).expand(-1, k)
            assert torch.equal(parent // (1 if h == 0 else k), users)
        print(f"{name} corpus, finite beams per level:", [c.tolist() for c in counts])
        assert bool((counts[1] >= counts[0]).all()) and bool((counts[2] >= counts[1]).all())
        assert int(counts[0].min()) >= 1
        if name == "sparse":
            assert int(counts[0].max()) <= 4 and int(counts[2].min()) > 4


# ---- generate against an exhaustive ranking of a 12-item corpus


@functools.lru_cache(maxsize=None)
def _exhaustive_case():
    from modules.model import EncoderDecoderRetrievalModel
    dev = torch.device("cuda")
    K, L, B = 16, 3, 8
    g = torch.Generator().manual_seed(12)
    torch.manual_seed(12)
    # 12 distinct rows with shared prefixes: few codes at the first two levels
    rows = torch.stack([torch.randint(0, 3, (60,), generator=g), torch.randint(0, 2, (60,), generator=g) + 5,
                        torch.randint(0, K, (60,), generator=g)], dim=1)
    corpus = torch.unique(rows, dim=0)[:12].contiguous()
    assert corpus.shape == (12, L)
    model = EncoderDecoderRetrievalModel(corpus, L, K, t5_d_model=64, t5_num_heads=2, t5_d_ff=128, t5_num_layers=2,
                                         top_k_for_generation=16).eval()
    with torch.no_grad():
        for lin in model.decoder_mlp:
            lin.weight.mul_(8.0)
    batch = synthetic_batch(corpus, B, 4, g, pad="b_mod_items")
    model64 = copy.deepcopy(model).double().eval()
    return model.to(dev), model64.to(dev), to_device(batch, dev), corpus.to(dev)


def _teacher_forced_sums(model, batch, corpus):
    """[B, N]: the sum over the levels of log_softmax(head_h(decoder state))[item id h], one decoder pass per item."""
    from modules.model import _strip_dedup_col
    L = model.num_hierarchies
    ids_in = _strip_dedup_col(batch.sem_ids, L + 1, L)
    mask = _strip_dedup_col(batch.seq_mask.long(), L + 1, L)
    sums = []
    with torch.no_grad():
        enc, enc_mask = model.encoder_forward_pass(mask, ids_in, batch.user_ids)
        B = enc.shape[0]
        for item in corpus:
            hid = model.decoder_forward_pass(future_ids=item.unsqueeze(0).expand(B, -1).contiguous(), encoder_output=enc,
                                             attention_mask_for_encoder=enc_mask)
            total = 0
            for h in range(L):
                total = total + torch.log_softmax(model.decoder_mlp[h](hid[:, h]), dim=-1)[:, item[h]]
            sums.append(total)
    return torch.stack(sums, dim=1)


def test_exact_generate_ranks_a_small_corpus_exhaustively():
    """k = 16 is at least the number of corpus prefixes at every level, so nothing is pruned: per user the finite beams
    are the 12 corpus items in descending order of their teacher-forced log-probability, the last 4 beams are -inf."""
    model, model64, batch, corpus = _exhaustive_case()
    N, B = corpus.shape[0], batch.sem_ids.shape[0]
    model.beam_impl = "exact"
    try:
        out = model.generate_next_sem_id(batch)
    finally:
        model.beam_impl = "sample"
    assert out.sem_ids.shape == (B, 16, 3) and out.log_probas.shape == (B, 16)
    assert bool(torch.isfinite(out.log_probas[:, :N]).all()) and bool((out.log_probas[:, N:] == float("-inf")).all())
    sums64 = _teacher_forced_sums(model64, batch, corpus)
    sums32 = _teacher_forced_sums(model, batch, corpus)
    sv, order = torch.sort(sums64, dim=1, descending=True, stable=True)
    skip = _near(sv[:, :-1], sv[:, 1:]).any(dim=1)
    print(f"exhaustive ranking: {int(skip.sum())}/{B} users with two items inside the {GAP:g} gap")
    # at most 2 of the 8 users may be skipped; with this seed the fp64 reference alone stays within it
    assert int(skip.sum()) <= 2
    ok = ~skip
    assert torch.equal(out.sem_ids[ok][:, :N], corpus[order][ok])
    gate("exhaustive log_probas", out.log_probas[ok][:, :N], torch.gather(sums32, 1, order)[ok], sv[ok], 4)


# ---- generate at the default config


@functools.lru_cache(maxsize=None)
def _default_case():
    dev = torch.device("cuda")
    return default_model_and_batch(dev)


def _cache_free_exact_generate(model, batch):
    """generate() under "exact" with every step decoded in full (BOS + all ids so far, no cache) and ref_topk_step."""
    from modules.model import _strip_dedup_col
    L, k = model.num_hierarchies, model.top_k_for_generation
    ids_in = _strip_dedup_col(batch.sem_ids, L + 1, L)
    mask = _strip_dedup_col(batch.seq_mask.long(), L + 1, L)
    idx = model._prefix_index_for_codebooks()
    with torch.no_grad():
        enc, enc_mask = model.encoder_forward_pass(mask, ids_in, batch.user_ids)
        ids = scores = None
        amb_any = torch.zeros(enc.shape[0], dtype=torch.bool, device=enc.device)
        for h in range(L):
            if h == 0:
                hid = model.decoder_forward_pass(encoder_output=enc, attention_mask_for_encoder=enc_mask)
            else:
                hid = model.decoder_forward_pass(future_ids=ids.reshape(-1, h),
                                                 encoder_output=enc.repeat_interleave(k, dim=0),
                                                 attention_mask_for_encoder=enc_mask.repeat_interleave(k, dim=0))
            logits = model.decoder_mlp[h](hid[:, -1])
            ids, scores64, _, _, amb = ref_topk_step(logits, scores, ids, idx._index, idx._corpus, k)
            scores = scores64.float()
            amb_any |= amb
    return ids, scores, amb_any


@functools.lru_cache(maxsize=None)
def _default_reference():
    model, batch = _default_case()
    return _cache_free_exact_generate(model, batch)


@pytest.mark.parametrize("attention", ["torch", "hip"])
def test_exact_generate_equals_cache_free_restatement_default_config(attention):
    from rqhip import ops
    model, batch = _default_case()
    L, k = model.num_hierarchies, model.top_k_for_generation
    B = batch.sem_ids.shape[0]
    r_ids, r_lp, amb = _default_reference()
    model.beam_impl, model.attention_impl = "exact", attention
    try:
        out = model.generate_next_sem_id(batch)
    finally:
        model.beam_impl, model.attention_impl = "sample", "torch"
    assert out.sem_ids.shape == (B, k, L) and out.log_probas.shape == (B, k)
    assert out.sem_ids.dtype == torch.int64 and out.log_probas.dtype == torch.float32
    n_amb = compare_beams(out.sem_ids, out.log_probas, None, r_ids, r_lp, None, amb, 1e-5, 1e-5)
    print(f"default config, attention {attention}: {n_amb}/{B} users inside the gap, "
          f"{int(torch.isfinite(r_lp).sum())} finite beams")
    assert n_amb <= B // 8
    # ids at ALL positions of the unambiguous users, the -inf ones included
    assert torch.equal(out.sem_ids[~amb], r_ids[~amb])
    fin = torch.isfinite(out.log_probas)
    assert fin.any()
    # every finite beam is a corpus item, and a user's finite beams are pairwise distinct
    valid = ops.prefix_lookup(model._prefix_index._index, model._prefix_index._corpus, out.sem_ids.reshape(-1, L))
    assert bool(valid.reshape(B, k)[fin].all())
    same = (out.sem_ids.unsqueeze(1) == out.sem_ids.unsqueeze(2)).all(dim=-1)               # [B, k, k]
    same &= fin.unsqueeze(1) & fin.unsqueeze(2) & ~torch.eye(k, dtype=torch.bool, device=fin.device)
    assert not bool(same.any())


# ---- no randomness (these fail without beam_impl)


def test_exact_generate_ignores_the_seed_and_leaves_the_generator_alone(monkeypatch):
    import modules.model as mm
    model, batch = _default_case()

    def never(probas):
        raise AssertionError("the exact search drew noise")

    model.beam_impl = "exact"
    try:
        monkeypatch.setattr(mm, "_exponential_like", never)
        torch.manual_seed(1)
        state = torch.cuda.get_rng_state()
        a = model.generate_next_sem_id(batch)
        assert torch.equal(torch.cuda.get_rng_state(), state)
        torch.manual_seed(2)
        b = model.generate_next_sem_id(batch)
    finally:
        model.beam_impl = "sample"
    assert torch.equal(a.sem_ids, b.sem_ids) and same_bits(a.log_probas, b.log_probas)


def test_the_default_search_still_draws_once_per_level(monkeypatch):
    import modules.model as mm
    model, batch = _default_case()
    calls = []
    orig = mm._exponential_like

    def counted(probas):
        calls.append(tuple(probas.shape))
        return orig(probas)

    assert model.beam_impl == "sample"
    monkeypatch.setattr(mm, "_exponential_like", counted)
    torch.manual_seed(1)
    state = torch.cuda.get_rng_state()
    model.generate_next_sem_id(batch)
    assert len(calls) == model.num_hierarchies
    assert not torch.equal(torch.cuda.get_rng_state(), state)


# ---- graph capture


def test_exact_generate_under_graph_capture_equals_eager():
    dev = torch.device("cuda")
    model, batch = default_model_and_batch(dev, B=32, N=5000, seed=3)
    model.beam_impl = "exact"
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
