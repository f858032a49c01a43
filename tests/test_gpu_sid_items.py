"""The item index and the one-launch expansion of beams to items (csrc/sid_items.hip) against the Python oracle of
tests/sid_items_cases.py.  Integer work and copied scores: every result is compared with torch.equal.

The corpus is the hand-made one of sid_items_cases: 40 rows, L = 3, codes < 4, groups of 30 (more than most n), 5, 2 and
three single rows, no group contiguous."""
import functools
import random

import pytest
import torch

import sid_items_cases as cases
from sid_items_cases import A, ABSENT, B5, C2, D, E, F, NEG_INF

pytestmark = pytest.mark.gpu

L = 3
NAN = float("nan")
NEGATIVE = (1, -2, 3)        # a beam with a negative id: no corpus row
PAD = [-1, -1, -1, -1]


@functools.lru_cache(maxsize=None)
def _corpus():
    return torch.tensor(cases.hand_corpus(), dtype=torch.int64, device="cuda")


@functools.lru_cache(maxsize=None)
def _index():
    from modules.sid_items import SemIdItemIndex
    return SemIdItemIndex(_corpus())


def _dev(rows, dtype=torch.int64):
    return torch.tensor(rows, dtype=dtype, device="cuda")


def _check(beams, scores, n, history=None, expand=None):
    """The kernel on lists against the oracle on the same lists -> (items, item_scores) of the kernel."""
    B, k = len(beams), len(beams[0])
    want_items, want_scores = cases.topn(cases.hand_corpus(), beams, scores, n, history)
    d_hist = None if history is None else _dev(history).reshape(B, -1)
    expand = expand or _index().expand
    items, item_scores = expand(_dev(beams).reshape(B, k, L), _dev(scores, torch.float32).reshape(B, k), n, d_hist)
    assert items.shape == (B, n) and items.dtype == torch.int64
    assert item_scores.shape == (B, n) and item_scores.dtype == torch.float32
    assert torch.equal(items, _dev(want_items)), (items.tolist(), want_items)
    assert torch.equal(item_scores, _dev(want_scores, torch.float32)), (item_scores.tolist(), want_scores)
    return items, item_scores


def _random_users(B, k, T, seed):
    """B users with k beams each from a pool that repeats tuples, misses the corpus and holds -inf / NaN scores; scores
    descend (multiples of 1/4, exact in fp32); T history items per user, some padding, some repeated."""
    rnd = random.Random(seed)
    pool = [A, B5, C2, D, E, F, ABSENT, NEGATIVE, B5, A]
    table = cases.hand_corpus()
    ranks = cases.dedup_ranks(table)
    beams, scores, history = [], [], []
    for u in range(B):
        beams.append([list(rnd.choice(pool)) for _ in range(k)])
        scores.append([rnd.choice([NEG_INF, NAN]) if rnd.random() < 0.2 else -0.25 * (b + u) for b in range(k)])
        row = []
        for _ in range(T):
            i = rnd.randrange(len(table))
            row += PAD if rnd.random() < 0.3 else table[i] + [ranks[i]]
        history.append(row)
    return beams, scores, history


@pytest.mark.parametrize("n", [1, 10, 256])
@pytest.mark.parametrize("k", [1, 10, 64])
def test_expand_matches_oracle_for_every_k_and_n(k, n):
    """B = 5 users on workgroups of 4: the last workgroup holds one user.  With n = 1 and n = 10 the group of 30 gives
    more items than n; with n = 256 every user has fewer than n."""
    for B, seed in ((1, 0), (5, 1), (4, 2)):
        beams, scores, history = _random_users(B, k, 6, seed * 100 + k + n)
        _check(beams, scores, n)
        _check(beams, scores, n, history)


def test_more_items_than_n_and_fewer():
    # one beam of 30 items, n = 10: the 10 lowest item numbers of the group; n = 256: all 30, then the tail
    items, _ = _check([[list(A)]], [[-1.0]], 10)
    group = [i for i, row in enumerate(cases.hand_corpus()) if tuple(row) == A]
    assert items[0].tolist() == group[:10]
    items, scores = _check([[list(A)]], [[-1.0]], 256)
    assert items[0, :30].tolist() == group and bool((items[0, 30:] == -1).all()) and bool((scores[0, 30:] == NEG_INF).all())
    # the cut falls inside a later beam's group: 5 + 2 + the first 3 of 30
    beams, scores = cases.pad_beams([B5, C2, A, D], [-0.5, -1.0, -1.5, -2.0], 10)
    items, _ = _check([beams], [scores], 10)
    assert items[0, 7:].tolist() == group[:3]


def test_dead_beams_nan_duplicates_and_tuples_outside_the_corpus():
    inf = NEG_INF
    beams = [
        cases.pad_beams([A, B5, C2, D], [inf, inf, -1.0, -2.0], 10),               # -inf beams at the front
        cases.pad_beams([B5, A, C2, D], [-1.0, inf, inf, -2.0], 10),               # in the middle
        cases.pad_beams([A, B5, C2, D], [inf] * 4, 10),                            # everywhere
        cases.pad_beams([B5, C2, D], [NAN, -1.0, -2.0], 10),                       # a NaN score contributes nothing
        cases.pad_beams([B5, C2, B5, D, C2], [-1.0, -2.0, -3.0, -4.0, -5.0], 10),  # the same tuple twice
        cases.pad_beams([B5, C2, B5, D], [inf, -2.0, -3.0, -4.0], 10),             # the earlier copy is dead: the later one gives
        cases.pad_beams([ABSENT, NEGATIVE, D, F], [-1.0, -2.0, -3.0, -4.0], 10),   # not in the corpus / a negative id
        cases.pad_beams([E, F], [float("inf"), 0.0], 10),                          # +inf is a score like any other
    ]
    items, scores = _check([b for b, _ in beams], [s for _, s in beams], 10)
    assert bool((items[2] == -1).all()) and bool((scores[2] == NEG_INF).all())
    assert int((items[4] >= 0).sum()) == 5 + 2 + 1 and int((items[5] >= 0).sum()) == 2 + 5 + 1
    assert int((items[6] >= 0).sum()) == 2


def _item_row(tuple_, rank):
    return list(tuple_) + [rank]


def test_history_cases():
    beams, scores = cases.pad_beams([B5, C2, D, A], [-1.0, -2.0, -3.0, -4.0], 10)
    n = 12
    histories = {
        "all padding": PAD * 4,
        "middle ranks of the group of 5": _item_row(B5, 1) + _item_row(B5, 2) + _item_row(B5, 3) + PAD,
        "a whole group": _item_row(C2, 1) + _item_row(C2, 0) + _item_row(D, 0) + PAD,
        "the same item twice": _item_row(B5, 0) + _item_row(B5, 0) + PAD + _item_row(B5, 0),
        "negative rank or id is padding": _item_row(B5, -1) + [0, -1, 2, 0] + _item_row(ABSENT, 0) + _item_row(B5, 7),
    }
    names = list(histories)
    B = len(names)
    items, _ = _check([beams] * B, [scores] * B, n, [histories[name] for name in names])
    table = cases.hand_corpus()
    b5 = [i for i, row in enumerate(table) if tuple(row) == B5]
    got = dict(zip(names, items.tolist()))
    assert got["all padding"][:5] == b5
    assert got["middle ranks of the group of 5"][:2] == [b5[0], b5[4]]
    c2_d = {i for i, row in enumerate(table) if tuple(row) in (C2, D)}
    assert not c2_d & set(got["a whole group"])
    assert got["the same item twice"][:4] == b5[1:]
    assert got["negative rank or id is padding"] == got["all padding"]
    # absent history, and T = 0
    plain, _ = _check([beams], [scores], n)
    assert plain[0].tolist() == got["all padding"]
    empty, _ = _index().expand(_dev([beams]), _dev([scores], torch.float32), n,
                               torch.zeros(1, 0, dtype=torch.int64, device="cuda"))
    assert torch.equal(empty, plain)


def test_history_longer_than_64_items():
    """The kernel keeps a lane's matching history items as a 64-bit mask and compares the items beyond the 64th in full:
    matches on both sides of that border, and beyond it alone."""
    beams, scores = cases.pad_beams([B5, C2, A, E], [-1.0, -2.0, -3.0, -4.0], 10)
    filler = [_item_row(D, 0), PAD, _item_row(F, 0), _item_row(ABSENT, 0)]
    both = [filler[j % 4] for j in range(70)]
    both[0], both[63], both[64], both[66], both[69] = (_item_row(B5, 4), _item_row(B5, 0), _item_row(B5, 2),
                                                       _item_row(C2, 1), _item_row(A, 3))
    beyond = [filler[j % 4] for j in range(70)]
    beyond[65], beyond[68], beyond[69] = _item_row(C2, 0), _item_row(A, 0), _item_row(A, 0)
    at_64 = [filler[j % 4] for j in range(64)]
    at_64[63] = _item_row(E, 0)
    flat = [[v for item in h for v in item] for h in (both, beyond)]
    items, _ = _check([beams] * 2, [scores] * 2, 12, flat)
    table = cases.hand_corpus()
    b5 = [i for i, row in enumerate(table) if tuple(row) == B5]
    c2 = [i for i, row in enumerate(table) if tuple(row) == C2]
    assert items[0, :3].tolist() == [b5[1], b5[3], c2[0]] and items[1, :6].tolist() == b5 + [c2[1]]
    _check([beams], [scores], 12, [[v for item in at_64 for v in item]])     # T = 64 exactly: the mask alone


def test_strided_history_and_strided_corpus_views():
    from rqhip import ops
    beams, scores, history = _random_users(5, 10, 6, 77)
    want, want_scores = _check(beams, scores, 10, history)
    # history as a column slice of a wider tensor whose other columns hold real items: ld_hist > T * (L + 1)
    wide = torch.cat([_dev(history), _dev([_item_row(A, 0) + _item_row(B5, 0)] * 5)], dim=1)
    view = wide[:, : 6 * (L + 1)]
    assert view.stride(0) == 8 * (L + 1)
    got, got_scores = _index().expand(_dev(beams), _dev(scores, torch.float32), 10, view)
    assert torch.equal(got, want) and torch.equal(got_scores, want_scores)
    # the corpus as the first L columns of the tokenizer's [N, L + 1] table: ld = L + 1
    ranks = _dev(cases.dedup_ranks(cases.hand_corpus()))
    table = torch.cat([_corpus(), ranks[:, None]], dim=1)
    corpus = table[:, :L]
    assert corpus.stride(0) == L + 1
    index = ops.sid_item_index_build(corpus, ranks)
    got, got_scores = ops.sid_items_topn(index, corpus, _dev(beams), _dev(scores, torch.float32), 10, _dev(history))
    assert torch.equal(got, want) and torch.equal(got_scores, want_scores)
    assert torch.equal(ops.sid_item_lookup(index, corpus, table), torch.arange(40, device="cuda"))


def test_items_of():
    from rqhip import ops
    rows = cases.hand_corpus()
    ranks = cases.dedup_ranks(rows)
    index = _index()
    # the ranks the index computed are the tokenizer's: a dedup_rank call as SemanticIdTokenizer.precompute_corpus_ids makes
    cached_ids = torch.cat([_corpus(), ops.dedup_rank(_corpus().t().contiguous(), 4)[0].unsqueeze(1)], dim=1)
    assert torch.equal(index.ranks, cached_ids[:, L]) and index.ranks.tolist() == ranks
    # every corpus row gives its own number
    assert torch.equal(index.items_of(cached_ids), torch.arange(40, device="cuda"))
    # (tuple, group size), an unknown tuple, a negative id and ranks no int32 holds give -1
    queries = [list(t) + [size] for t, size in cases.GROUP_SIZES.items()]
    queries += [list(ABSENT) + [0], list(NEGATIVE) + [0], list(A) + [-1], list(A) + [2 ** 32], list(A) + [2 ** 31]]
    got = index.items_of(_dev(queries))
    assert got.tolist() == [-1] * len(queries) == cases.items_of(rows, queries)
    mixed = [list(A) + [29], list(B5) + [4], list(C2) + [2], list(F) + [0]]
    assert index.items_of(_dev(mixed)).tolist() == cases.items_of(rows, mixed)
    assert index.items_of(torch.zeros(0, L + 1, dtype=torch.int64, device="cuda")).shape == (0,)


def test_same_bits_on_every_run_and_on_a_second_index():
    from modules.sid_items import SemIdItemIndex
    beams, scores, history = _random_users(5, 64, 6, 5)
    args = (_dev(beams), _dev(scores, torch.float32), 50, _dev(history))
    first = _index().expand(*args)
    again = _index().expand(*args)
    other = SemIdItemIndex(_corpus().clone()).expand(*args)
    for got in (again, other):
        assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1])


def test_the_kernel_writes_the_tails_itself():
    """Through the raw binding, with the output buffers preset to garbage: every element is written by the one launch."""
    from rqhip import _lib, ops
    index = _index()
    B, k, n = 5, 10, 40
    beams = [cases.pad_beams([D, C2], [-1.0, -2.0], k), cases.pad_beams([], [], k), cases.pad_beams([A], [-1.0], k),
             cases.pad_beams([ABSENT], [-1.0], k), cases.pad_beams([A, B5, C2, D, E, F], [-1.0] * 6, k)]
    d_beams = _dev([b for b, _ in beams])
    d_scores = _dev([s for _, s in beams], torch.float32)
    items = torch.full((B, n), 123456789, dtype=torch.int64, device="cuda")
    item_scores = torch.full((B, n), 7.0, dtype=torch.float32, device="cuda")
    rc = _lib.lib().rqhip_sid_items_topn(index._index.data_ptr(), index._index.numel(), index._corpus.data_ptr(), 40, L, L,
                                         d_beams.data_ptr(), d_scores.data_ptr(), B, k, None, 0, 0, n, items.data_ptr(),
                                         item_scores.data_ptr(), ops._stream())
    assert rc == 0
    want_items, want_scores = cases.topn(cases.hand_corpus(), [b for b, _ in beams], [s for _, s in beams], n)
    assert torch.equal(items, _dev(want_items)) and torch.equal(item_scores, _dev(want_scores, torch.float32))
    counts = (items >= 0).sum(dim=1).tolist()
    assert counts == [3, 0, 30, 0, 40]
    for u, c in enumerate(counts):
        assert bool((items[u, c:] == -1).all()) and bool((item_scores[u, c:] == NEG_INF).all())
