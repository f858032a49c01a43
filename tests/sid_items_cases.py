"""What the item-expansion tests share: the oracle of rqhip_sid_items_topn and rqhip_sid_item_lookup in plain Python
(dicts and loops over lists, no torch operator on the hot logic) and the hand-made corpus and cases.

Test infrastructure like tests/retrieval_cases.py: imported by the tests only; the product package never imports it."""
NEG_INF = float("-inf")

# ---- the oracle


def dedup_ranks(rows):
    """rank[i] = the number of earlier rows with row i's tuple (the tokenizer's dedup column)."""
    seen, out = {}, []
    for row in rows:
        key = tuple(row)
        out.append(seen.get(key, 0))
        seen[key] = out[-1] + 1
    return out


def item_map(rows):
    """{(tuple, rank): item number}."""
    return {(tuple(row), r): i for i, (row, r) in enumerate(zip(rows, dedup_ranks(rows)))}


def items_of(rows, ids):
    """ids: rows of L + 1 numbers, tuple and rank -> item numbers, -1 where the corpus has no such row."""
    table = item_map(rows)
    return [table.get((tuple(q[:-1]), q[-1]), -1) for q in ids]


def history_items(history_row, L):
    """The non-padding (tuple, rank) pairs of one user's history row of T * (L + 1) numbers."""
    out = set()
    for j in range(0, len(history_row), L + 1):
        item = history_row[j:j + L + 1]
        if all(v >= 0 for v in item):
            out.add((tuple(item[:L]), item[L]))
    return out


def topn(rows, beams, scores, n, history=None):
    """beams [B][k][L], scores [B][k] (floats; -inf and NaN allowed), history None or [B][T * (L + 1)] ->
    (items [B][n], item_scores [B][n]) as include/rqhip.h states them."""
    table = item_map(rows)
    L = len(rows[0]) if rows else (len(beams[0][0]) if beams and beams[0] else 0)
    all_items, all_scores = [], []
    for u, (ubeams, uscores) in enumerate(zip(beams, scores)):
        seen_items = history_items(history[u], L) if history is not None else set()
        out, used = [], set()
        for beam, score in zip(ubeams, uscores):
            if len(out) == n:
                break
            if not score > NEG_INF:           # -inf and NaN
                continue
            key = tuple(beam)
            if key in used:
                continue
            used.add(key)
            r = 0
            while len(out) < n:
                item = table.get((key, r))
                if item is None:
                    break
                if (key, r) not in seen_items:
                    out.append((item, score))
                r += 1
        pad = n - len(out)
        all_items.append([i for i, _ in out] + [-1] * pad)
        all_scores.append([s for _, s in out] + [NEG_INF] * pad)
    return all_items, all_scores


# ---- the hand-made corpus: L = 3, codes < 4, 40 rows; groups of 30 (A), 5 (B), 2 (C) and three single rows (D, E, F);
# F shares A's first two ids.  Row i of the corpus is LAYOUT[i * 7 % 40], so that no group is contiguous.

A, B5, C2, D, E, F = (1, 2, 3), (0, 1, 2), (3, 3, 0), (2, 0, 1), (0, 0, 0), (1, 2, 0)
ABSENT = (3, 0, 3)          # a tuple no corpus row has (its prefix 3 is C2's)
LAYOUT = [A] * 30 + [B5] * 5 + [C2] * 2 + [D, E, F]
GROUP_SIZES = {A: 30, B5: 5, C2: 2, D: 1, E: 1, F: 1}


def hand_corpus():
    return [list(LAYOUT[i * 7 % 40]) for i in range(40)]


def pad_beams(tuples, scores, k):
    """k beams: the given ones, then -inf beams of tuple E."""
    assert len(tuples) == len(scores) <= k
    extra = k - len(tuples)
    return [list(t) for t in tuples] + [list(E)] * extra, list(scores) + [NEG_INF] * extra
