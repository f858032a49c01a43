"""`model.encoder_rows = "packed"` (modules/model.py): `forward` on the valid encoder tokens only, against the padded
fused path on the same batch.

Model: d_model 64, 2 heads, d_ff 96, 2 layers, K = 16, L = 3, batch 5 with histories of 4, 3, 2, 1 and 4 items out of
4 slots (retrieval_cases.synthetic_batch, pad = "b_mod_items"), with and without a user token: encoder bound 16 / 17,
N = 56 / 61 packed tokens, decoder T = 4.

Eval mode: every row-local kernel is batch-independent by contract (include/rqhip.h) and the packed attention keeps the
padded bits (tests/test_gpu_t5_attention_packed.py), so loss and loss_d are torch.equal to the padded fused ones, under
grad and under no_grad, with the operator projections, the grouped ones and the bf16 matrix arithmetic.  Weight
gradients sum over the rows in other groups of 16 / 32 rows, so they are gated: per parameter e = max|g - g64| /
max|g64| against the operator model in fp64 on the padded batch, e_packed <= 4 e_padded_fused -- the factor
tests/test_gpu_t5_attention.py gives two fp32 summation orders -- and exact zero where the fp64 gradient is exactly zero.

Train mode (dropout 0.1): the gate and thresholds of tests/test_gpu_train_replay.py against the operator model fed the
step's own masks, the packed kernels' masks scattered to the padded positions."""
import contextlib
import copy
import functools

import pytest
import torch

from retrieval_cases import (LAYERS, Call, Site, err, gate, loss_and_grads, recording, replay_step, same_bits, setting,
                             synthetic_batch, to_device, _train_step)

pytestmark = pytest.mark.gpu

B, ITEMS, L, K = 5, 4, 3, 16
COUNTS = [4, 3, 2, 1, 4]                       # pad = "b_mod_items": the last b % 4 items of row b are padding
FUSED = dict(attention="hip_train", norm="hip", ffn="hip", head="hip", embed="hip")
SETTINGS = {"fused": (FUSED, "fp32"), "proj": ({**FUSED, "proj": "hip"}, "fp32"), "bf16": ({**FUSED, "proj": "hip"}, "bf16")}
STEP_SEED, DRAW_SEED = 21, 5


def _counted(batch, counts=None):
    """The batch as a CountedSeqBatch: item_counts from its own mask (on the host), or as given."""
    from data.schemas import CountedSeqBatch
    if counts is None:
        counts = batch.seq_mask.view(batch.seq_mask.shape[0], -1, L + 1)[:, :, 0].sum(1).cpu()
    return CountedSeqBatch(*batch, item_counts=counts.to(torch.int64))


@functools.lru_cache(maxsize=None)
def _models(user):
    """(fp32 model on the device, its fp64 copy on the host, the counted batch on the device, the plain one on both)."""
    from modules.model import EncoderDecoderRetrievalModel
    g = torch.Generator().manual_seed(31)
    torch.manual_seed(31)
    corpus = torch.randint(0, K, (200, L), generator=g)
    model = EncoderDecoderRetrievalModel(corpus, L, K, t5_d_model=64, t5_num_heads=2, t5_d_ff=96, t5_num_layers=LAYERS,
                                         num_user_bins=10 if user else None)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("layer_norm.weight"):
                p.copy_(1 + 0.5 * torch.randn(p.shape, generator=g))
    host = synthetic_batch(corpus, B, ITEMS, g, pad="b_mod_items")
    model64 = copy.deepcopy(model).double().eval()
    plain = to_device(host, "cuda")
    counted = _counted(plain)
    assert counted.item_counts.tolist() == COUNTS
    return model.cuda().eval(), model64, counted, plain, host


@functools.lru_cache(maxsize=None)
def _reference(user):
    _, model64, _, _, host = _models(user)
    return loss_and_grads(model64, host)


@contextlib.contextmanager
def _rows(model, rows, arith="fp32"):
    model.encoder_rows, model.matmul_arith = rows, arith
    try:
        yield model
    finally:
        model.encoder_rows, model.matmul_arith = "padded", "fp32"
        model._push_attention_impl()


ATTENTION_OPS = ("t5_attention", "t5_attention_fwd_train", "t5_attention_bwd", "t5_attention_packed",
                 "t5_attention_packed_fwd_train", "t5_attention_packed_bwd", "rows_pack", "rows_unpack")


@contextlib.contextmanager
def _spy():
    """Counts the calls of the attention ops, padded and packed, and of the pack / unpack ops."""
    from rqhip import ops
    calls = dict.fromkeys(ATTENTION_OPS, 0)
    with pytest.MonkeyPatch.context() as mp:
        for name in calls:
            def counted(*a, _name=name, _real=getattr(ops, name), **kw):
                calls[_name] += 1
                return _real(*a, **kw)
            mp.setattr(ops, name, counted)
        yield calls


def _step(model, batch):
    model.zero_grad(set_to_none=True)
    out = model(batch)
    out.loss.backward()
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    return out.loss.detach(), out.loss_d.detach(), grads


@pytest.mark.parametrize("name", list(SETTINGS))
@pytest.mark.parametrize("user", [False, True], ids=["no user token", "user token"])
def test_eval_mode_keeps_the_loss_bits_and_gates_the_gradients(user, name):
    model, _, batch, _, _ = _models(user)
    loss64, grads64 = _reference(user)
    choices, arith = SETTINGS[name]
    with setting(model.eval(), **choices):
        with _rows(model, "padded", arith), _spy() as calls:
            with torch.no_grad():
                quiet_p = model(batch)
            loss_p, loss_d_p, grads_p = _step(model, batch)
            assert calls["t5_attention_packed"] == calls["t5_attention_packed_fwd_train"] == calls["rows_pack"] == 0
        with _rows(model, "packed", arith), _spy() as calls:
            with torch.no_grad():
                quiet = model(batch)
            loss, loss_d, grads = _step(model, batch)
            # the encoder's self-attentions and the decoder's cross-attentions are packed calls, once per mode
            assert calls["t5_attention_packed"] == calls["t5_attention_packed_fwd_train"] == 2 * LAYERS
            assert calls["t5_attention_packed_bwd"] == 2 * LAYERS and calls["rows_pack"] == 2
            assert calls["rows_unpack"] == 1                                  # the pack's backward
    assert torch.equal(quiet.loss, quiet_p.loss) and torch.equal(quiet.loss_d, quiet_p.loss_d)
    assert torch.equal(loss, loss_p) and torch.equal(loss_d, loss_d_p)
    assert sorted(grads) == sorted(grads_p) == sorted(grads64) and len(grads) > 40
    worst = 0.0
    for n in sorted(grads):
        assert torch.isfinite(grads[n]).all(), n
        if not bool(grads64[n].any()):
            print(f"{name}: grad {n}: the fp64 reference is exactly zero")
            assert not bool(grads[n].any()) and not bool(grads_p[n].any()), n
            continue
        e_packed, e_padded = err(grads[n], grads64[n]), err(grads_p[n], grads64[n])
        ratio = e_packed / e_padded if e_padded > 0 else (0.0 if e_packed == 0 else float("inf"))
        worst = max(worst, ratio)
        print(f"{name}: grad {n}: e_packed {e_packed:.3e} e_padded {e_padded:.3e} ratio {ratio:.2f}")
        assert e_packed <= 4 * e_padded, n
    print(f"{name}, user token {user}: largest ratio e_packed / e_padded {worst:.2f}")


def _calls_of(model, batch, grad):
    with _spy() as calls:
        if grad:
            loss = _step(model, batch)[0]
        else:
            with torch.no_grad():
                loss = model(batch).loss
    return loss, calls


def test_dispatch():
    model, _, counted, plain, _ = _models(False)
    packed_ops = ("t5_attention_packed", "t5_attention_packed_fwd_train", "t5_attention_packed_bwd", "rows_pack",
                  "rows_unpack")
    g = torch.Generator().manual_seed(2)
    long = _counted(to_device(synthetic_batch(model.codebooks.cpu(), 2, 65, g, pad="row1"), "cuda"))   # 260 tokens
    with setting(model.eval(), **FUSED):
        want_long, today_long = _calls_of(model, long, False)
        want, today = _calls_of(model, counted, True)                          # the default attribute: today's calls
        assert all(today[n] == 0 for n in packed_ops)
        assert today["t5_attention_fwd_train"] == today["t5_attention_bwd"] == 3 * LAYERS
        with _rows(model, "packed"):
            loss, calls = _calls_of(model, counted, True)
            assert torch.equal(loss, want)
            assert calls["t5_attention_packed_fwd_train"] == calls["t5_attention_packed_bwd"] == 2 * LAYERS
            assert calls["t5_attention_fwd_train"] == calls["t5_attention_bwd"] == LAYERS   # the decoder's self-attention
            assert calls["t5_attention"] == calls["t5_attention_packed"] == 0
            loss, calls = _calls_of(model, counted, False)
            assert torch.equal(loss, want)
            assert calls["t5_attention_packed"] == 2 * LAYERS and calls["t5_attention"] == LAYERS
            # a plain TokenizedSeqBatch: nothing says how long the rows are
            loss, calls = _calls_of(model, plain, True)
            assert torch.equal(loss, want) and calls == today
            # a row without a token (count 0, no user token) would change meaning: the padded path
            empty = plain._replace(sem_ids=plain.sem_ids.clone(), seq_mask=plain.seq_mask.clone())
            empty.sem_ids[2], empty.seq_mask[2] = -1, False
            want_empty, _ = _calls_of(model, empty, True)
            loss, calls = _calls_of(model, _counted(empty), True)
            assert _counted(empty).item_counts.tolist() == [4, 3, 0, 1, 4]
            assert torch.equal(loss, want_empty) and calls == today
            # a bound beyond the short kernel's 256: the forward falls back as it does today (operators)
            loss, calls = _calls_of(model, long, False)
            assert torch.equal(loss, want_long) and calls == today_long and all(calls[n] == 0 for n in packed_ops)
        # attention_impl = "torch": the operators, no fused attention at all
        with setting(model, **{**FUSED, "attention": "torch"}), _rows(model, "packed"):
            loss, calls = _calls_of(model, counted, True)
            assert torch.isfinite(loss) and all(v == 0 for n, v in calls.items())
    # with a user token a row without items still has one token: packed
    model_u, _, counted_u, plain_u, _ = _models(True)
    empty = plain_u._replace(sem_ids=plain_u.sem_ids.clone(), seq_mask=plain_u.seq_mask.clone())
    empty.sem_ids[2], empty.seq_mask[2] = -1, False
    with setting(model_u.eval(), **FUSED):
        want, _ = _calls_of(model_u, empty, True)
        with _rows(model_u, "packed"):
            loss, calls = _calls_of(model_u, _counted(empty), True)
            assert torch.equal(loss, want) and calls["t5_attention_packed_fwd_train"] == 2 * LAYERS
            with pytest.raises(ValueError, match="item_counts"):
                model_u(_counted(empty, torch.tensor([1, 2])))
        model_u.encoder_rows = "ragged"
        try:
            with pytest.raises(ValueError, match="encoder_rows"):
                model_u(counted_u)
        finally:
            model_u.encoder_rows = "padded"


# ---- train mode


@contextlib.contextmanager
def _packed_attention_sites(log):
    """recording()'s spy for the packed attention: the mask of a call is the padded index law's,
    ops.t5_attention_dropout_keep(seed, B, H, Tq bound, Tk bound, p)."""
    from rqhip import ops
    real_fwd, real_bwd = ops.t5_attention_packed_fwd_train, ops.t5_attention_packed_bwd

    def bounds(q, kw):
        groups = kw["cu_k"].numel() - 1
        return groups, (kw["max_q"] if kw.get("cu_q") is not None else q.shape[1]), kw["max_k"]

    def fwd(q, k, v, n_heads, **kw):
        p, seed = kw.get("p", 0.0), kw.get("seed")
        value = None if seed is None else int(seed)
        log.calls.append(Call("attention", "fwd", value, (p,), (q.shape, k.shape, v.shape)))
        if p > 0:
            groups, Tq, Tk = bounds(q, kw)
            log.sites.append(Site("attention", float(p), ops.t5_attention_dropout_keep(seed, groups, n_heads, Tq, Tk, p),
                                  value))
        return real_fwd(q, k, v, n_heads, **kw)

    def bwd(q, k, v, out, lse, d_out, n_heads, **kw):
        seed = kw.get("seed")
        log.calls.append(Call("attention", "bwd", None if seed is None else int(seed), (kw.get("p", 0.0),),
                              (q.shape, k.shape, v.shape)))
        return real_bwd(q, k, v, out, lse, d_out, n_heads, **kw)

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "t5_attention_packed_fwd_train", fwd)
        mp.setattr(ops, "t5_attention_packed_bwd", bwd)
        yield


def _scatter(keep, valid):
    """A row-local mask of the N packed rows [1, N, c] at the padded positions [B, T, c]; padded positions: all True
    (they do not reach the loss)."""
    full = torch.ones(valid.shape + keep.shape[-1:], dtype=torch.bool, device=keep.device)
    full[valid.to(keep.device)] = keep[0]
    return full


def _valid(user):
    tokens = torch.tensor(COUNTS) * (L + 1) + int(user)
    T = ITEMS * (L + 1) + int(user)
    return torch.arange(T)[None, :] < tokens[:, None]


@functools.lru_cache(maxsize=None)
def _train(user):
    """One packed fused train-mode step (loss, gradients, the log with its masks scattered to the padded positions) and
    its replays on the operators on the padded batch, in fp32 and in fp64."""
    model, model64, counted, plain, host = _models(user)
    valid = _valid(user)
    N = int(valid.sum())
    with setting(model.eval(), **FUSED, proj="hip"), _rows(model, "packed"):
        with recording(DRAW_SEED) as log, _packed_attention_sites(log):
            loss, grads = _train_step(model, counted, STEP_SEED)
        again = _train_step(model, counted, STEP_SEED)
    sites = [s._replace(keep=_scatter(s.keep, valid)) if (s.kind != "attention" and tuple(s.keep.shape[:2]) == (1, N))
             else s for s in log.sites]
    scattered = type(log)(sites, log.calls)
    with setting(model):
        ref32 = replay_step(model, plain, scattered)
    ref64 = replay_step(model64, host, scattered)
    return loss, grads, again, log, scattered, ref32, ref64


def test_train_mode_same_seed_same_bits():
    loss, grads, (loss2, grads2), log, _, _, _ = _train(True)
    assert same_bits(loss, loss2) and sorted(grads) == sorted(grads2)
    assert all(same_bits(grads[n], grads2[n]) for n in grads)
    # 2 * LAYERS packed and LAYERS padded attention calls, each with a seed of its own and its backward's
    fwd = [c for c in log.fused("fwd") if c.op == "attention"]
    bwd = [c for c in log.fused("bwd") if c.op == "attention"]
    assert len(fwd) == len(bwd) == 3 * LAYERS and len({c.seed for c in fwd}) == len(fwd)
    assert sorted(c.seed for c in fwd) == sorted(c.seed for c in bwd)


def test_train_mode_against_fp64_with_the_step_s_own_masks():
    user = True
    loss, grads, _, log, scattered, (loss32, grads32), (loss64, grads64) = _train(user)
    sites = (2 + 4 * LAYERS) + (2 + 6 * LAYERS)
    assert len(log) == len(scattered) == sites and all(s.p == 0.1 for s in log.sites)
    valid = _valid(user)
    N, T = int(valid.sum()), valid.shape[1]
    # the encoder's row-local sites were recorded on the N packed rows and replayed on the padded positions
    enc = log.sites[:2 + 4 * LAYERS]
    assert all(tuple(s.keep.shape[:2]) == (1, N) for s in enc if s.kind != "attention")
    assert all(tuple(s.keep.shape) == (B, 2, T, T) for s in enc if s.kind == "attention")
    assert all(tuple(s.keep.shape[:2]) == (B, T) for s in scattered.sites[:2 + 4 * LAYERS] if s.kind != "attention")
    cross = [s for s in log.sites[2 + 4 * LAYERS:] if s.kind == "attention"][1::2]
    assert all(tuple(s.keep.shape) == (B, 2, L + 1, T) for s in cross)
    assert sorted(grads) == sorted(grads32) == sorted(grads64) and len(grads) > 40
    gate("packed: loss", loss.reshape(1), loss32.reshape(1), loss64.reshape(1), 4)
    for n in sorted(grads):
        gate(f"packed: grad {n}", grads[n], grads32[n], grads64[n], 8)


def test_a_scattered_mask_of_another_seed_fails_the_gate():
    """The control: the glue mask behind the encoder's first self-attention rebuilt from another seed, scattered the same
    way, in the reference alone.  Against that reference the packed step's gradients must miss the gate."""
    from test_gpu_t5_add_norm import _masks
    user = True
    model, model64, _, plain, host = _models(user)
    _, grads, _, log, scattered, _, _ = _train(user)
    valid = _valid(user)
    i = 2
    s = log.sites[i]
    assert s.kind == "glue_in" and log.sites[i - 1].kind == "attention"
    N, d = s.keep.shape[1], s.keep.shape[2]
    keep = _masks(s.seed + 1, N, d, s.p, 0.0)[0].view(s.keep.shape).to(s.keep.device)
    assert not torch.equal(keep, s.keep)
    wrong = scattered.swapped(i, _scatter(keep, valid))
    with setting(model.eval()):
        _, grads32 = replay_step(model, plain, wrong)
    _, grads64 = replay_step(model64, host, wrong)
    missed = []
    for n in sorted(grads):
        try:
            gate(f"site {i} of another seed: grad {n}", grads[n], grads32[n], grads64[n], 8)
        except AssertionError:
            missed.append(n)
    print(f"{len(missed)} of {len(grads)} gradients miss the gate against the wrong reference")
    assert missed


# ---- the loader and train_decoder


def _loader_set(subsample):
    from data.processed import RecDataset, SeqData
    from modules.tokenizer.semids import SemanticIdTokenizer
    n_items, w = 300, L + 1
    ds = SeqData(root=f"synthetic:{n_items}", dataset=RecDataset.AMAZON, is_train=True, subsample=subsample).to_device("cuda")
    tok = SemanticIdTokenizer(input_dim=16, output_dim=8, hidden_dims=[16], codebook_size=K, n_layers=L, n_cat_feats=0)
    tok.cached_ids = torch.randint(0, K, (n_items, w), generator=torch.Generator().manual_seed(3)).cuda()
    return ds, tok


def _same_batch(a, b):
    assert type(a)._fields == type(b)._fields
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(x, y)


@pytest.mark.parametrize("subsample", [True, False])
def test_loader_host_windows(subsample):
    from data.schemas import CountedSeqBatch, TokenizedSeqBatch
    from data.seq_loader import TokenizedSeqLoader
    ds, tok = _loader_set(subsample)
    S, Bl = ds.max_seq_len, 32
    loader = TokenizedSeqLoader(ds, tok, Bl, shuffle=True, host_windows=True)
    torch.manual_seed(8)
    device_state = torch.cuda.get_rng_state()
    first = list(loader)
    assert torch.equal(torch.cuda.get_rng_state(), device_state)            # the draws are the host generator's
    assert len(first) == len(loader) == -(-len(ds) // Bl)
    fill = []
    for b in first:
        assert isinstance(b, CountedSeqBatch) and isinstance(b, TokenizedSeqBatch)
        rows = b.sem_ids.shape[0]
        assert not b.item_counts.is_cuda and b.item_counts.dtype == torch.int64 and b.item_counts.shape == (rows,)
        items = b.seq_mask.view(rows, S, L + 1)
        assert bool((items == items[:, :, :1]).all())                        # an item is valid or padding as a whole
        valid = items[:, :, 0].cpu()
        assert torch.equal(valid.sum(1), b.item_counts)
        assert torch.equal(valid, torch.arange(S)[None, :] < b.item_counts[:, None])   # and the valid items a prefix
        fill.append(b.item_counts.float().mean().item() / S)
    print(f"subsample {subsample}: fill of the epoch's batches {sum(fill) / len(fill):.3f}")
    seen = torch.cat([b.user_ids[:, 0] for b in first]).cpu()
    assert torch.equal(seen.sort().values, ds.userId.cpu().sort().values) and not torch.equal(seen, ds.userId.cpu())
    torch.manual_seed(8)
    for a, b in zip(first, loader):                                         # the seed reproduces the epoch
        _same_batch(a, b)
        assert torch.equal(a.item_counts, b.item_counts)


@pytest.mark.parametrize("subsample", [True, False])
def test_loader_without_host_windows_is_today_s(subsample):
    from data.schemas import TokenizedSeqBatch
    from data.seq_loader import TokenizedSeqLoader
    from rqhip import ops
    ds, tok = _loader_set(subsample)
    S, Bl = ds.max_seq_len, 32
    torch.manual_seed(8)
    host_state = torch.get_rng_state()
    got = list(TokenizedSeqLoader(ds, tok, Bl, shuffle=True))
    after = torch.cuda.get_rng_state()
    assert torch.equal(torch.get_rng_state(), host_state)                   # no host draw
    assert all(type(b) is TokenizedSeqBatch for b in got)
    # an epoch is one randperm on the device, then per batch one randint (training rows) and the kernel
    torch.manual_seed(8)
    perm = torch.randperm(len(ds), device="cuda")
    for i, b in enumerate(got):
        rows = perm[i * Bl:(i + 1) * Bl]
        draws = torch.randint(0, 2 ** 62, (rows.shape[0], 2), dtype=torch.int64, device="cuda") if subsample else None
        _same_batch(b, ops.seq_batch(ds, rows, tok.cached_ids, S, draws))
    assert torch.equal(torch.cuda.get_rng_state(), after)


def test_train_decoder_packed(tmp_path):
    import train_decoder
    from data.processed import RecDataset
    from modules.model import EncoderDecoderRetrievalModel
    root = str(tmp_path) + "/"
    cfg = dict(dataset_folder="synthetic:300", dataset=RecDataset.AMAZON, batch_size=16, iterations=4, partial_eval_every=2,
               full_eval_every=4, log_every=1, learning_rate=0.001, weight_decay=0.0001, max_grad_norm=1.0,
               vae_input_dim=768, vae_hidden_dims=[32], vae_embed_dim=16, vae_codebook_size=16, vae_n_layers=3,
               vae_n_cat_feats=0, t5_d_model=64, t5_num_heads=2, t5_d_ff=128, t5_num_layers=2, top_k_for_generation=10,
               top_k_eval_list=[1, 5, 10], save_dir_root=root)
    gin = train_decoder.gin
    gin.clear_config()
    try:      # the line configs/decoder_amazon_packed.gin adds: `train`'s own parameter set is pinned
        gin.parse_config('encoder_rows.mode = "packed"')
        with _spy() as calls:
            torch.manual_seed(0)
            out = train_decoder.train(**cfg)
    finally:
        gin.clear_config()
    users = 150
    evals = 2 * -(-users // 16)                                              # two partial evals over the eval split
    assert [it for it, _ in out["losses"]] == [0, 1, 2, 3] and all(v == v and abs(v) != float("inf") for _, v in out["losses"])
    assert len(out["eval_losses"]) == 2 and all(v == v for _, v in out["eval_losses"])
    # every training and partial-eval forward ran packed: the synthetic histories hold at least one item
    assert calls["t5_attention_packed_fwd_train"] == calls["t5_attention_packed_bwd"] == 4 * 2 * 2
    assert calls["t5_attention_packed"] == evals * 2 * 2 and calls["rows_pack"] == 4 + evals
    state = torch.load(out["checkpoint"], map_location="cpu", weights_only=False)
    fresh = EncoderDecoderRetrievalModel(torch.zeros_like(state["model"]["codebooks"]), 3, 16, t5_d_model=64, t5_num_heads=2,
                                         t5_d_ff=128, t5_num_layers=2)
    fresh.load_state_dict(state["model"], strict=True)
    assert fresh.encoder_rows == "padded" and not any("encoder_rows" in k for k in state["model"])
    with _spy() as calls:          # without the binding: the padded path
        torch.manual_seed(0)
        train_decoder.train(**{**cfg, "iterations": 1, "partial_eval_every": 100, "full_eval_every": 100})
    assert calls["rows_pack"] == calls["t5_attention_packed_fwd_train"] == 0 and calls["t5_attention_fwd_train"] == 6
