"""The item expansion on the host: the argument checks of the four rqhip_sid_item* symbols (all of them run before any
HIP call), the ops' errors on host tensors, the entry point (recommend.recommend, configs/decoder_amazon_recommend.gin)
and the Python oracle of tests/sid_items_cases.py on a case worked by hand.  No GPU needed."""
import ctypes
import inspect
import os

import pytest
import torch

import sid_items_cases as cases

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rq-vae-recommender_amd")

ONE = 1     # any non-null pointer: no check dereferences it, and no call here gets as far as a launch


def _index(l, N=0):
    need = l.rqhip_sid_item_index_bytes(N)
    buf = ctypes.create_string_buffer(need)
    return buf, ctypes.addressof(buf), need


def _build(l, *, corpus=ONE, N=5, L=3, ld=3, rank=ONE, index=None, index_bytes=0):
    return l.rqhip_sid_item_index_build(corpus, N, L, ld, rank, index, index_bytes, None)


def _lookup(l, *, index=None, index_bytes=0, corpus=ONE, N=0, L=3, ld=3, ids=ONE, P=4, ld_ids=4, items=ONE):
    return l.rqhip_sid_item_lookup(index, index_bytes, corpus, N, L, ld, ids, P, ld_ids, items, None)


def _topn(l, *, index=None, index_bytes=0, corpus=ONE, N=0, L=3, ld=3, beams=ONE, scores=ONE, B=4, k=10, history=None, T=0,
          ld_hist=0, n=10, items=ONE, item_scores=ONE):
    return l.rqhip_sid_items_topn(index, index_bytes, corpus, N, L, ld, beams, scores, B, k, history, T, ld_hist, n, items,
                                  item_scores, None)


def test_index_bytes():
    from rqhip import _lib
    l = _lib.lib()
    assert l.rqhip_sid_item_index_bytes(-1) == 0
    # 2 x N slots (a power of two, at least 64) and N ranks, 4 bytes each: 12 to 20 bytes per item
    assert l.rqhip_sid_item_index_bytes(1000) == (2048 + 1000) * 4
    assert l.rqhip_sid_item_index_bytes(0) == 64 * 4
    assert l.rqhip_sid_item_index_bytes(12101) == (32768 + 12101) * 4


def test_index_build_argument_checks_without_gpu():
    from rqhip import _lib
    l = _lib.lib()
    err = l.rqhip_last_error
    buf, ptr, need = _index(l, 5)
    assert _build(l, corpus=None, index=ptr, index_bytes=need) == -1 and b"corpus null" in err()
    assert _build(l, ld=2, index=ptr, index_bytes=need) == -1 and b"ld >= L" in err()
    assert _build(l, L=0, ld=3, index=ptr, index_bytes=need) == -1 and b"L >= 1" in err()
    assert _build(l, L=16, ld=16, index=ptr, index_bytes=need) == -2 and b"RQHIP_MAX_PREFIX_LEN" in err()
    assert _build(l, N=1 << 30, index=ptr, index_bytes=need) == -2 and b"2^30" in err()
    assert _build(l, rank=None, index=ptr, index_bytes=need) == -1 and b"null rank" in err()
    assert _build(l) == -3 and b"index buffer too small" in err()
    assert _build(l, index=ptr, index_bytes=need - 1) == -3 and b"index buffer too small" in err()


def test_item_lookup_argument_checks_without_gpu():
    from rqhip import _lib
    l = _lib.lib()
    err = l.rqhip_last_error
    buf, ptr, need = _index(l)
    ok = dict(index=ptr, index_bytes=need)
    assert _lookup(l, corpus=None, N=5, **ok) == -1 and b"corpus null" in err()
    assert _lookup(l, ld=2, **ok) == -1 and b"ld >= L" in err()
    assert _lookup(l, L=16, ld=16, ld_ids=17, **ok) == -2 and b"RQHIP_MAX_PREFIX_LEN" in err()
    assert _lookup(l, ld_ids=3, **ok) == -1 and b"ld_ids >= L + 1" in err()        # no room for the rank
    assert _lookup(l, ids=None, **ok) == -1 and b"bad query" in err()
    assert _lookup(l, items=None, **ok) == -1 and b"bad query" in err()
    assert _lookup(l, P=-1, **ok) == -1 and b"bad query" in err()
    assert _lookup(l, P=0) == -3 and b"index buffer too small" in err()
    assert _lookup(l, P=0, index=ptr, index_bytes=need - 1) == -3 and b"index buffer too small" in err()
    assert _lookup(l, P=0, ids=None, items=None, **ok) == 0                          # nothing to do: no launch


def test_items_topn_argument_checks_without_gpu():
    from rqhip import _lib
    l = _lib.lib()
    err = l.rqhip_last_error
    buf, ptr, need = _index(l)
    ok = dict(index=ptr, index_bytes=need)
    assert _topn(l, corpus=None, N=5, **ok) == -1 and b"corpus null" in err()
    assert _topn(l, ld=2, **ok) == -1 and b"ld >= L" in err()
    assert _topn(l, L=16, ld=16, **ok) == -2 and b"RQHIP_MAX_PREFIX_LEN" in err()
    assert _topn(l, k=0, **ok) == -1 and b"1 <= k <= 64" in err()
    assert _topn(l, k=65, **ok) == -2 and b"1 <= k <= 64" in err()
    assert _topn(l, n=0, **ok) == -1 and b"1 <= n <= 256" in err()
    assert _topn(l, n=257, **ok) == -2 and b"1 <= n <= 256" in err()
    assert _topn(l, T=-1, **ok) == -1 and b"T >= 0" in err()
    assert _topn(l, history=ONE, T=20, ld_hist=79, **ok) == -1 and b"ld_hist >= T * (L + 1)" in err()
    for name in ("beams", "scores", "items", "item_scores"):
        assert _topn(l, **{name: None}, **ok) == -1 and b"bad arguments" in err()
    assert _topn(l, B=0) == -3 and b"index buffer too small" in err()
    assert _topn(l, B=0, index=ptr, index_bytes=need - 1) == -3 and b"index buffer too small" in err()
    assert _topn(l, B=0, **ok) == 0                                                  # nothing to do: no launch
    assert _topn(l, B=0, k=64, n=256, history=ONE, T=20, ld_hist=80, **ok) == 0
    assert l.rqhip_version() == 462


def test_ops_reject_host_tensors():
    from rqhip import ops
    from rqhip._lib import RqHipError
    corpus = torch.tensor(cases.hand_corpus())
    rank = torch.tensor(cases.dedup_ranks(cases.hand_corpus()))
    index = torch.zeros(16, dtype=torch.uint8)
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.sid_item_index_build(corpus, rank)
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.sid_item_lookup(index, corpus, torch.zeros(2, 4, dtype=torch.long))
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.sid_items_topn(index, corpus, torch.zeros(2, 10, 3, dtype=torch.long), torch.zeros(2, 10), 10)
    assert list(inspect.signature(ops.sid_items_topn).parameters) == ["index", "corpus", "beams", "scores", "n", "history"]
    from modules.sid_items import SemIdItemIndex
    idx = SemIdItemIndex(corpus)                       # a host corpus: nothing is built until a device is named
    assert idx.num_items == 40 and idx._index is None
    with pytest.raises(RqHipError, match="no CPU fallback"):
        idx.items_of(torch.zeros(2, 4, dtype=torch.long))
    with pytest.raises(ValueError, match="int64"):
        SemIdItemIndex(corpus.float())


def test_model_has_recommend_items_and_keeps_its_state_dict():
    from modules.model import ItemRecommendation
    from retrieval_cases import tiny_model
    from rqhip._lib import RqHipError
    assert ItemRecommendation._fields == ("items", "scores", "sem_ids", "log_probas")
    model = tiny_model()
    names = list(model.state_dict())
    params = inspect.signature(model.recommend_items).parameters
    assert list(params) == ["batch", "n_items", "exclude_history"]
    assert params["n_items"].default is None and params["exclude_history"].default is True
    from retrieval_cases import tiny_batch
    with pytest.raises(RqHipError, match="ROCm device tensors"):       # generate's own error: there is no CPU path
        model.recommend_items(tiny_batch())
    assert list(model.state_dict()) == names


def test_recommend_signature_is_evaluates_plus_three():
    import evaluate_decoder
    import recommend
    ev = inspect.signature(evaluate_decoder.evaluate).parameters
    rec = inspect.signature(recommend.recommend).parameters
    own = dict(n_items=10, exclude_history=True, output_path=None)
    assert list(rec) == list(ev) + list(own)
    for name, p in ev.items():
        assert rec[name].default == p.default, name
    for name, default in own.items():
        assert rec[name].default == default, name
    doc = " ".join(recommend.__doc__.split())
    assert "targets_in_history" in doc and "can then not be hit at the item level" in doc


def test_recommend_config_binds_only_recommend_and_agrees_with_the_eval_config():
    import recommend
    from data.processed import RecDataset
    from rqhip import ginlite
    params = inspect.signature(recommend.recommend).parameters

    def bindings(name):
        ginlite.clear_config()
        try:
            ginlite.parse_config_file(os.path.join(PKG, "configs", name))
            return {scope: dict(b) for scope, b in ginlite._BINDINGS.items()}
        finally:
            ginlite.clear_config()

    got = bindings("decoder_amazon_recommend.gin")
    assert set(got) == {"recommend"}
    bound = got["recommend"]
    assert set(bound) <= set(params)
    assert bound["dataset"] is RecDataset.AMAZON and bound["n_items"] == 10 and bound["exclude_history"] is True
    ev = bindings("decoder_amazon_eval.gin")["evaluate"]
    shared = set(bound) & set(ev)
    assert {"checkpoint_path", "batch_size", "beam_impl", "top_k_for_generation", "vae_hidden_dims", "vae_codebook_size",
            "t5_d_model", "t5_num_layers", "dataset_folder", "pretrained_rqvae_path", "attention_impl"} <= shared
    assert {n: bound[n] for n in shared} == {n: ev[n] for n in shared}


# ---- the oracle on a case worked by hand: every number below was written down from the corpus, not computed


def test_oracle_on_a_case_worked_by_hand():
    X, Y, Z = (1, 1, 1), (2, 2, 2), (3, 3, 3)
    #        0  1  2  3  4  5  6      X is items 0, 2, 5 (ranks 0, 1, 2); Y is items 1, 4 (ranks 0, 1); Z is items 3, 6
    rows = [X, Y, X, Z, Y, X, Z]
    assert cases.dedup_ranks(rows) == [0, 0, 1, 0, 1, 2, 1]
    assert cases.items_of(rows, [X + (0,), X + (2,), X + (3,), Y + (1,), (9, 9, 9, 0), Z + (-1,)]) == [0, 5, -1, 4, -1, -1]
    inf, nan = float("inf"), float("nan")
    # user 0: Y then X then Y again (skipped) then an unknown tuple then Z; n = 6 cuts Z's second item
    # user 1: a -inf beam in front, a NaN beam, then Z; only Z's two items come out
    # user 2: everything -inf
    beams = [[Y, X, Y, (0, 0, 0), Z], [X, Y, Z, Z, Z], [X, Y, Z, X, Y]]
    scores = [[-1.0, -2.0, -3.0, -4.0, -5.0], [-inf, nan, -1.5, -2.5, -3.5], [-inf] * 5]
    items, got = cases.topn(rows, beams, scores, 6)
    assert items == [[1, 4, 0, 2, 5, 3], [3, 6, -1, -1, -1, -1], [-1] * 6]
    assert got == [[-1.0, -1.0, -2.0, -2.0, -2.0, -5.0], [-1.5, -1.5, -inf, -inf, -inf, -inf], [-inf] * 6]
    # history: user 0 has seen item 4 (Y, 1) and item 2 (X, 1), the latter twice, and a padded item; user 1 has seen a
    # whole group (Z); user 2 nothing but padding.  An item with a negative rank is padding too.
    pad = (-1, -1, -1, -1)
    history = [list(Y + (1,) + X + (1,) + pad + X + (1,)), list(Z + (0,) + Z + (1,) + pad + X + (-1,)), list(pad * 4)]
    items, got = cases.topn(rows, beams, scores, 6, history)
    assert items == [[1, 0, 5, 3, 6, -1], [-1] * 6, [-1] * 6]
    assert got == [[-1.0, -2.0, -2.0, -5.0, -5.0, -inf], [-inf] * 6, [-inf] * 6]
    # n = 1: the best contributing beam's first item that is not in the history
    assert cases.topn(rows, beams, scores, 1, history)[0] == [[1], [-1], [-1]]
    # a wrong oracle would not pass: the same call without the duplicate rule gives another list
    assert cases.topn(rows, [[Y, X, Y]], [[-1.0, -2.0, -3.0]], 7)[0] == [[1, 4, 0, 2, 5, -1, -1]]


def test_hand_corpus_is_what_the_tests_say():
    rows = cases.hand_corpus()
    assert len(rows) == 40 and all(len(r) == 3 and all(0 <= v < 4 for v in r) for r in rows)
    sizes = {}
    for r in rows:
        sizes[tuple(r)] = sizes.get(tuple(r), 0) + 1
    assert sizes == cases.GROUP_SIZES and sorted(sizes.values()) == [1, 1, 1, 2, 5, 30]
    assert cases.ABSENT not in sizes
    first = [i for i, r in enumerate(rows) if tuple(r) == cases.A]
    assert first != list(range(first[0], first[0] + 30))        # the big group is not contiguous
