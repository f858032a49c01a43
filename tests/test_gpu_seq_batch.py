"""ops.seq_batch (csrc/seq_batch.hip), SemanticIdTokenizer.tokenize_rows and data/seq_loader.py against code that was
already in the tree: for given rows and draws the SeqBatch is built on the host with data.processed.seq_window, moved to
the device and passed through SemanticIdTokenizer.forward; every field of the one-launch batch must be torch.equal to
that, with the same dtypes and shapes."""
import functools

import pytest
import torch

from retrieval_cases import impls, same_bits, small_model

pytestmark = pytest.mark.gpu

N_ITEMS = 37
BIG = 2 ** 62
SMALL = (11, 128, True)         # the set-up of tests/test_gpu_t5_norm_impl.py


@functools.lru_cache(maxsize=None)
def _tokenizer(w):
    """A tokenizer whose cached ids are a random [N_ITEMS, w] table set by hand: no RQ-VAE run is needed."""
    from modules.tokenizer.semids import SemanticIdTokenizer
    tok = SemanticIdTokenizer(input_dim=16, output_dim=8, hidden_dims=[16], codebook_size=16, n_layers=w - 1, n_cat_feats=0)
    g = torch.Generator().manual_seed(100 + w)
    tok.cached_ids = torch.randint(0, 1000, (N_ITEMS, w), generator=g).cuda()
    return tok


def _lengths(S):
    return [0, 1, 2, 3, S - 1, S, S + 1, 3 * S]


@functools.lru_cache(maxsize=None)
def _users(S):
    """(histories, future items, user ids) with every edge length in one set."""
    g = torch.Generator().manual_seed(7 * S)
    hists = [torch.randint(0, N_ITEMS, (n,), generator=g).tolist() for n in _lengths(S)]
    futs = torch.randint(0, N_ITEMS, (len(hists),), generator=g).tolist()
    return hists, futs, [500 + 3 * i for i in range(len(hists))]


def _seq_data(hists, futs, users, S, subsample):
    from data.processed import RecDataset, SeqData
    offsets = torch.zeros(len(hists) + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(torch.tensor([len(h) for h in hists]), 0)
    store = {"userId": torch.tensor(users), "offsets": offsets, "items": torch.tensor([i for h in hists for i in h], dtype=torch.int64),
             "itemId_fut": torch.tensor(futs)}
    ds = SeqData("/nonexistent", dataset={20: RecDataset.AMAZON, 200: RecDataset.ML_1M}.get(S, RecDataset.AMAZON),
                 sequences={"train": store}, subsample=subsample)
    ds._max_seq_len = S          # (S = 2 is no dataset's length: the kernel's smallest)
    return ds.to_device("cuda")


def _rows_and_draws(hists, S, B):
    """Row b reads user b % U with its draws at one of the four corners of the two ranges (shortest and longest window
    from the first start, and from the last start, where the end of the sequence clips it), some of them shifted by a
    multiple of the range to just below 2^62."""
    rows, draws = [], []
    for b in range(B):
        r = b % len(hists)
        m0, m1 = max(0, len(hists[r]) + 1 - 3) + 1, S - 1
        u0, u1 = ((0, 0), (0, m1 - 1), (m0 - 1, m1 - 1), (m0 - 1, 0))[(b // len(hists) + b) % 4]
        if b % 3 == 1:
            u0, u1 = u0 + m0 * ((BIG - 1 - u0) // m0), u1 + m1 * ((BIG - 1 - u1) // m1)
        rows.append(r)
        draws.append((u0, u1))
    return rows, draws


def _reference(tok, hists, futs, users, rows, draws, S, bad=()):
    """SemanticIdTokenizer.forward on the SeqBatch that seq_window describes.  A padded position holds item 0 with a
    False mask (forward overwrites it with -1; the reference's -1 is no row of the table).  Item ids in `bad` are looked
    up as item 0 and their slots set to padding afterwards."""
    from data.processed import seq_window
    from data.schemas import SeqBatch
    ids, fut, uid = [], [], []
    for b, r in enumerate(rows):
        seq = hists[r] + [futs[r]]
        u0, u1 = draws[b] if draws is not None else (0, 0)
        first, count, fut_pos = seq_window(len(hists[r]), u0, u1, S, draws is not None)
        ids.append(seq[first:first + count] + [-1] * (S - count))
        fut.append([seq[fut_pos]])
        uid.append([users[r]])
    ids, fut = torch.tensor(ids).cuda(), torch.tensor(fut).cuda()
    off = torch.zeros_like(ids, dtype=torch.bool)
    off_fut = torch.zeros_like(fut, dtype=torch.bool)
    for v in bad:
        off |= ids == v
        off_fut |= fut == v
    mask = (ids >= 0) & ~off
    out = tok(SeqBatch(user_ids=torch.tensor(uid).cuda(), ids=ids.masked_fill(~mask, 0), ids_fut=fut.masked_fill(off_fut, 0),
                       x=None, x_fut=None, seq_mask=mask))
    if bad:
        out = out._replace(sem_ids_fut=out.sem_ids_fut.masked_fill(off_fut, -1))
    return out


def _same(got, want):
    for name in want._fields:
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert torch.equal(g, w), name


@pytest.mark.parametrize("B", [1, 3, 70])
@pytest.mark.parametrize("S", [2, 20, 200])
@pytest.mark.parametrize("w", [2, 4, 5, 9])
def test_one_launch_batch_equals_tokenizer_forward(w, S, B):
    from rqhip import ops
    tok = _tokenizer(w)
    hists, futs, users = _users(S)
    ds = _seq_data(hists, futs, users, S, True)
    rows, draws = _rows_and_draws(hists, S, B)              # B = 70: every user nine times, every corner of every user
    rows_d, draws_d = torch.tensor(rows).cuda(), torch.tensor(draws, dtype=torch.int64).cuda()
    got = ops.seq_batch(ds, rows_d, tok.cached_ids, S, draws_d)
    assert got.user_ids.shape == (B, 1) and got.sem_ids.shape == (B, S * w) and got.seq_mask.dtype == torch.bool
    _same(got, _reference(tok, hists, futs, users, rows, draws, S))
    _same(ops.seq_batch(ds, rows_d, tok.cached_ids, S, draws_d), got)         # the same bits again
    # the same histories without subsampling: the last S items and the stored future item
    plain = ops.seq_batch(ds, rows_d, tok.cached_ids, S)
    _same(plain, _reference(tok, hists, futs, users, rows, None, S))
    # token_types=False leaves the two constant tensors out and nothing else
    bare = ops.seq_batch(ds, rows_d, tok.cached_ids, S, draws_d, token_types=False)
    assert bare.token_type_ids is None and bare.token_type_ids_fut is None
    _same(bare._replace(token_type_ids=got.token_type_ids, token_type_ids_fut=got.token_type_ids_fut), got)


def test_tokenize_rows_draws_on_the_device_and_needs_the_cache():
    from modules.tokenizer.semids import SemanticIdTokenizer
    from rqhip import ops
    tok, S = _tokenizer(4), 20
    hists, futs, users = _users(S)
    rows = torch.tensor([7, 7, 0, 5, 7]).cuda()
    train, plain = _seq_data(hists, futs, users, S, True), _seq_data(hists, futs, users, S, False)
    torch.manual_seed(5)
    got = tok.tokenize_rows(train, rows)
    torch.manual_seed(5)
    draws = torch.randint(0, 2 ** 62, (5, 2), dtype=torch.int64, device="cuda")
    _same(got, ops.seq_batch(train, rows, tok.cached_ids, S, draws))
    _same(got, _reference(tok, hists, futs, users, rows.tolist(), draws.tolist(), S))
    _same(tok.tokenize_rows(plain, rows), _reference(tok, hists, futs, users, rows.tolist(), None, S))
    _same(tok.tokenize_rows(plain, rows, draws), got)                           # explicit draws win
    empty = SemanticIdTokenizer(input_dim=16, output_dim=8, hidden_dims=[16], codebook_size=16, n_layers=3, n_cat_feats=0)
    with pytest.raises(RuntimeError, match="precompute_corpus_ids"):
        empty.tokenize_rows(train, rows)


@pytest.mark.parametrize("w", [4, 5])
def test_ids_outside_the_table_are_padding(w):
    """An id equal to n_items and an id of -5, with the table a view into the middle of a larger tensor: a missed clamp
    reads a wrong value inside the allocation."""
    from rqhip import ops
    S, pad_rows = 20, 8
    g = torch.Generator().manual_seed(9)
    big = torch.randint(1000, 2000, (N_ITEMS + 2 * pad_rows, w), generator=g).cuda()
    tok = _tokenizer(w)
    table = big[pad_rows:pad_rows + N_ITEMS]
    table.copy_(tok.cached_ids)
    hists, futs, users = (list(map(list, _users(S)[0])), list(_users(S)[1]), _users(S)[2])
    hists[3][1] = N_ITEMS
    hists[5][0], hists[5][7], hists[5][19] = -5, N_ITEMS, -5
    hists[7][-1], hists[7][-20] = N_ITEMS, -5
    futs[2], futs[6] = N_ITEMS, -5
    ds = _seq_data(hists, futs, users, S, True)
    rows, draws = _rows_and_draws(hists, S, 32)
    rows_d, draws_d = torch.tensor(rows).cuda(), torch.tensor(draws, dtype=torch.int64).cuda()
    for d, dd in ((draws, draws_d), (None, None)):
        got = ops.seq_batch(ds, rows_d, table, S, dd)
        want = _reference(tok, hists, futs, users, rows, d, S, bad=(N_ITEMS, -5))
        _same(got, want)
        assert int((~want.seq_mask).sum()) > 0 and bool((got.sem_ids[~got.seq_mask] == -1).all())
        assert bool((got.sem_ids < 1000).all()) and bool((got.sem_ids_fut < 1000).all())      # nothing from outside the view
    assert bool((got.sem_ids_fut[torch.tensor(rows) == 2] == -1).all())


def test_a_misaligned_even_table_takes_the_narrow_form():
    from rqhip import ops
    w, S = 4, 20
    tok = _tokenizer(w)
    flat = torch.zeros(N_ITEMS * w + 1, dtype=torch.int64, device="cuda")
    table = flat[1:].view(N_ITEMS, w)                     # 8 bytes past a 16-byte boundary
    table.copy_(tok.cached_ids)
    assert table.data_ptr() % 16 == 8
    hists, futs, users = _users(S)
    ds = _seq_data(hists, futs, users, S, True)
    rows, draws = _rows_and_draws(hists, S, 32)
    rows_d, draws_d = torch.tensor(rows).cuda(), torch.tensor(draws, dtype=torch.int64).cuda()
    _same(ops.seq_batch(ds, rows_d, table, S, draws_d), ops.seq_batch(ds, rows_d, tok.cached_ids, S, draws_d))


def test_rows_outside_the_users_give_empty_rows():
    from rqhip import ops
    w, S = 4, 20
    tok = _tokenizer(w)
    hists, futs, users = _users(S)
    ds = _seq_data(hists, futs, users, S, False)
    got = ops.seq_batch(ds, torch.tensor([len(hists), 5, -1]).cuda(), tok.cached_ids, S)
    for b in (0, 2):
        assert bool((got.sem_ids[b] == -1).all()) and not bool(got.seq_mask[b].any())
        assert bool((got.sem_ids_fut[b] == -1).all()) and int(got.user_ids[b, 0]) == -1
    _same(type(got)(*[t[1:2] for t in got]), _reference(tok, hists, futs, users, [5], None, S))


def _loader_set(B, subsample):
    S, U = 20, 2 * B + 3
    g = torch.Generator().manual_seed(21)
    hists = [torch.randint(0, N_ITEMS, (int(n),), generator=g).tolist() for n in torch.randint(0, 3 * S, (U,), generator=g)]
    futs = torch.randint(0, N_ITEMS, (U,), generator=g).tolist()
    users = [1000 + i for i in range(U)]
    return hists, futs, users, _seq_data(hists, futs, users, S, subsample)


def test_loader_epochs():
    from data.seq_loader import TokenizedSeqLoader
    from data.utils import cycle
    from rqhip import ops
    B, S = 4, 20
    tok = _tokenizer(4)
    hists, futs, users, ds = _loader_set(B, True)
    loader = TokenizedSeqLoader(ds, tok, B, shuffle=True)
    assert len(loader) == 3
    torch.manual_seed(8)
    first = list(loader)
    assert [b.user_ids.shape[0] for b in first] == [B, B, 3]
    seen = torch.cat([b.user_ids[:, 0] for b in first]).tolist()
    assert sorted(seen) == users and seen != users                       # every user once, in another order
    torch.manual_seed(8)
    for a, b in zip(first, loader):
        _same(b, a)                                                      # the seed reproduces the epoch
    # an epoch is one randperm, then per batch one randint and the kernel on views of the permutation
    torch.manual_seed(8)
    perm = torch.randperm(len(users), device="cuda")
    for i, b in enumerate(first):
        rows = perm[i * B:(i + 1) * B]
        draws = torch.randint(0, 2 ** 62, (rows.shape[0], 2), dtype=torch.int64, device="cuda")
        _same(b, ops.seq_batch(ds, rows, tok.cached_ids, S, draws))
        _same(b, _reference(tok, hists, futs, users, rows.tolist(), draws.tolist(), S))
    assert first[0].token_type_ids.data_ptr() == first[1].token_type_ids.data_ptr()     # written once per batch size
    # without shuffling the users come in order, with no draw on the way
    plain = _loader_set(B, False)[3]
    ordered = TokenizedSeqLoader(plain, tok, B, shuffle=False)
    state = torch.cuda.get_rng_state()
    batches = list(ordered)
    assert torch.equal(torch.cuda.get_rng_state(), state)
    assert torch.cat([b.user_ids[:, 0] for b in batches]).tolist() == users
    for i, b in enumerate(batches):
        _same(b, _reference(tok, hists, futs, users, list(range(i * B, min((i + 1) * B, len(users)))), None, S))
    # under data.utils.cycle the epochs follow each other
    it = cycle(loader)
    assert [next(it).user_ids.shape[0] for _ in range(5)] == [B, B, 3, B, B]
    # the constructor's one-time range check
    with pytest.raises(ValueError, match="outside"):
        short = _tokenizer(5)
        short_cache = short.cached_ids
        try:
            short.cached_ids = short_cache[:N_ITEMS - 30]
            TokenizedSeqLoader(ds, short, B)
        finally:
            short.cached_ids = short_cache


@pytest.mark.parametrize("embed", ["hip", "torch"])
def test_model_forward_accepts_a_loader_batch(embed):
    from data.seq_loader import TokenizedSeqLoader
    from modules.tokenizer.semids import SemanticIdTokenizer
    model = small_model(*SMALL)[0]
    L, K = model.num_hierarchies, model.num_embeddings_per_hierarchy
    tok = SemanticIdTokenizer(input_dim=16, output_dim=8, hidden_dims=[16], codebook_size=K, n_layers=L, n_cat_feats=0)
    corpus = model.codebooks.cuda()
    tok.cached_ids = torch.cat([corpus, torch.arange(corpus.shape[0], device="cuda").unsqueeze(1) % 3], dim=1)
    B, S = 4, 20
    g = torch.Generator().manual_seed(2)
    n = corpus.shape[0]
    hists = [torch.randint(0, n, (int(k),), generator=g).tolist() for k in (0, 1, 5, 19, 20, 21, 60, 3, 2, 30, 7)]
    futs = torch.randint(0, n, (len(hists),), generator=g).tolist()
    users = list(range(len(hists)))
    ds = _seq_data(hists, futs, users, S, True)
    torch.manual_seed(4)
    batches = list(TokenizedSeqLoader(ds, tok, B, shuffle=True))
    torch.manual_seed(4)
    perm = torch.randperm(len(users), device="cuda")
    with impls(model.eval()):
        model.embed_impl = embed
        try:
            with torch.no_grad():
                for i, batch in enumerate(batches):
                    rows = perm[i * B:(i + 1) * B]
                    draws = torch.randint(0, 2 ** 62, (rows.shape[0], 2), dtype=torch.int64, device="cuda")
                    built = _reference(tok, hists, futs, users, rows.tolist(), draws.tolist(), S)
                    got, want = model(batch).loss, model(built).loss
                    assert bool(torch.isfinite(got)) and same_bits(got, want)
        finally:
            model.embed_impl = "torch"
