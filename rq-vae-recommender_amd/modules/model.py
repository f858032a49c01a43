"""Generative retrieval model (TIGER): a T5 encoder over a user's semantic-id history, a T5 decoder that emits the
next item's ids one hierarchy level at a time.  API and state dict of the reference's modules/model.py
(EncoderDecoderRetrievalModel), so a checkpoint trained there loads here with strict=True.

The T5 body runs on torch operators, or on fused HIP calls chosen by four plain attributes that are handed to both
stacks whenever they are run: `model.attention_impl` ("torch", the default, "hip" or "hip_train"), `model.norm_impl`,
`model.ffn_impl` and `model.proj_impl` ("torch", the default, or "hip"; the last groups the attention projections, the
cross-attention K/V of `generate` and the K/V its decode steps write into the cache included).  What each replaces and
when it is taken: modules/t5.py.
`model.attention_long_impl` ("torch", the default, or "hip") goes to both stacks with them: with "hip" beside a fused
`attention_impl`, an attention call beyond the 256 tokens of csrc/t5_attention.hip is a call of
csrc/t5_attention_long.hip (up to 2048 tokens) instead of the operators, call by call (modules/t5.py).
`model.matmul_arith` ("fp32", the default, or "bf16"), `model.weight_images` ("none", the default, or "bf16") and
`model.saved_activations` ("fp32", the default, or "bf16") go to both stacks with them: which form the "hip" feed-forward
and the "hip" projections take -- bf16 operands with fp32 accumulation and storage, weights read from bf16 images that each
stack keeps current with one refresh launch per change of the weights, the feed-forward's two saved activations as bf16
images under grad.  The last two act on the "bf16" arithmetic alone and keep every bit of it; none of the three has an
effect on the "torch" bodies, nor on the attention, the norms, the heads or the embedding, which stay fp32
(modules/t5.py: matmul_forms).  train_decoder.train has no parameter for the last two.
`model.attention_arith` ("fp32", the default, or "bf16") goes to both stacks with them: the arithmetic of the long
attention calls that `attention_long_impl` = "hip" takes (bf16 matrix operands, fp32 softmax and storage; modules/t5.py),
`generate`'s cross-attention included.  The short kernel and the cached decode step stay fp32.  It is set on the model:
train_decoder.train has no parameter for it.
All nine are validated against modules/t5.py's STACK_ATTRIBUTES whenever they are handed over.
`model.head_impl = "hip"` (default "torch") makes the loss of `forward` -- the num_hierarchies heads and their
cross-entropy losses -- ONE autograd.SidHeadLossFunction call (csrc/sid_head_loss.hip): one call forward, one backward,
on the decoder's unsliced output and batch.sem_ids_fut as they are, with the decoder_mlp weights as separate pointers
(the state dict is unchanged).  It is taken when the decoder output is an fp32 device tensor and the shape is supported
(ops.sid_head_loss_supported), under grad and under no_grad and with every attention_impl / norm_impl; otherwise the
operators run, silently.  `generate` has its own head and is not affected.
`model.embed_impl = "hip"` (default "torch") makes the front that turns semantic ids into a stack's inputs_embeds -- the
level offsets, the mask product, the table gather, the separator, the user / BOS row and the mask that goes with them --
ONE autograd.SidEmbedFunction call per stack (csrc/sid_embed.hip): one launch forward, one backward, in
`encoder_forward_pass` and in `decoder_forward_pass` (without a cache).  `forward` hands both the batch's tensors as
they are, dedup column included, with that column skipped by the kernel's column stride.  It is taken when the ids and
the fp32 parameters are on the device and the shape is supported (`hip_embed_active`), under grad and under no_grad,
and by the encoder pass of `generate`; otherwise the operators run, silently.  inputs_embeds has the operators' bits;
the encoder's returned attention mask is then a bool tensor with the operators' truth values.  An id outside the table,
a device assert of the operators, reads a clamped row and gets no gradient.  The per-step lookup of `generate` is not
affected.
`model.encoder_rows = "packed"` (default "padded"; a model-level attribute like head_impl, not in the state dict, any
other value raises ValueError in `forward`) makes `forward` run the encoder on the VALID tokens only.  A training row is
padded to max_seq_len items, and the training window law rarely fills it (fill 0.36 on the synthetic histories), yet
every sub-layer runs on every padded slot, although padding never reaches the loss.  With "packed" the front's output
[B, T, d] is packed to [N, d], N the batch's valid tokens, by one launch (ops.rows_pack, csrc/rows_pack.hip; its
backward, ops.rows_unpack, carries the gradient back to the front, which is unchanged), the encoder stack runs on
[1, N, d] with its attention reading the rows through a cumulative-length table, and the decoder's cross-attention
reads the packed encoder output (modules/t5.py, "Packed rows").  N must be known on the host WITHOUT reading the
device -- a sync per step would stop the host from running ahead -- so `forward` packs only when the batch says how
many items each row holds: a data.schemas.CountedSeqBatch (`item_counts`, int64 CPU [B]: the leading valid item slots of
each row), as data/seq_loader.py yields with host_windows=True.  It also needs the fused attention to apply to both
stacks (`T5Stack.packed_rows_active`: attention_impl "hip_train", or "hip" under no_grad; bound within 256 tokens), a row
width that is a multiple of 4, and at least one token in every row: a row with no item and no user token would attend
uniformly over its padding in the padded form, which has no packed counterpart.  Otherwise -- a plain
TokenizedSeqBatch, host tensors, attention_impl = "torch", a longer history, an empty row -- `forward` runs the padded
path, silently, like every other *_impl.  In eval mode loss and loss_d have the padded fused path's bits; in train mode
the row-local dropout masks are another sample of the same law.  Measurements: profiles/packed_rows.txt.
`generate(..., item_counts=)`, and through it `generate_next_sem_id(batch)` and `recommend_items(batch)` on a
CountedSeqBatch, run packed by the same attribute and the same plan (`packed_rows_plan`, asked with the decode step's query
length 1): the front's output is packed by one ops.rows_pack launch, the encoder runs on [1, N, d], `cross_kv` projects
those N rows, and every decode step is `dec(x, cross_kv=..., decode_cache=slabs, encoder_packed=rows)` without an encoder
mask, whose cross-attention is ONE ops.t5_attention_packed_beams call per block: the k beams of a user read that user's
packed row (modules/t5.py, "Packed rows").  The cached self-attention stays on the slabs.  The returned ids and log
probabilities have the padded run's bits under both beam searches and every *_impl / *_arith attribute.  The same
fallbacks apply, silently, and one more: where the decode cache's slabs are not taken (`hip_attention_active`), the padded
path runs.  A packed `generate` cannot be captured into a graph, because N depends on the data.  Measurements:
profiles/packed_generate.txt.
Each hierarchy step of `generate` is the decoder on one new token per beam, the head's F.linear and ONE HIP launch
(ops.beam_step, csrc/beam_step.hip) that does the reference's softmax, multinomial sampling, log, prefix-validity
mask, sort and gathers.  After the encoder nothing is read back to
the host and no allocation depends on data, so a whole padded `generate` can be captured into a graph (a packed one
cannot: the number N of its encoder rows depends on the data).

Sampling: the reference's `torch.multinomial(probas, n, replacement=False)` is ATen's exponential race
`topk(p / q, n)` with `q = empty_like(p).exponential_(1)`.  `_exponential_like` draws the same q from the same
generator, so a seeded `generate` consumes the RNG as the reference's does.

`model.beam_impl = "exact"` (default "sample", the search above, unchanged in bits and in RNG use) makes `generate` the
deterministic constrained beam search: at every level EVERY corpus-valid child of every kept beam is scored, and the k
best are kept, by ONE ops.beam_topk_step launch per step (csrc/beam_step.hip) in place of the noise draw and
ops.beam_step.  A child's score is its parent's score plus the log-softmax value (x - max) - log(sum exp(x - max)) of its
code, in fp32 -- a log-softmax value, which unlike the sampling step's log(softmax) does not underflow to -inf for an
unlikely code.  Equal scores (-inf included) go to the lower candidate number beam * K + code, i.e. the stable
descending sort of a user's [beams * K] scores, so the whole output is determined: no noise is drawn, no generator is
touched, and two calls return the same bits.  It needs k <= K (not k <= n_cands).  A beam it reports as -inf means
"fewer than k corpus items share the kept prefixes": every kept finite beam is a corpus prefix and so has at least one
valid child, hence with a finite parent the search never loses a beam to chance, and a user's number of finite beams
never decreases from level to level.  Everything around the step -- encoder, cross K/V, the decode caches reordered by
the step's parent rows, the head, every *_impl / *_arith attribute, the returned shapes and dtypes -- is the same, and
the call is capturable into a graph with no noise baked in.  Any other value raises ValueError at `generate`.

`recommend_items(batch)` names items: one `generate_next_sem_id` call, then ONE launch (modules/sid_items.py,
csrc/sid_items.hip) that expands each user's beams, best first, to the corpus items that carry those tuples -- several
items can share a tuple, in ascending item number -- without the items of the user's own history, cut at n_items.  The
item index is cached beside the prefix index by the same rule and is no part of the state dict; `generate`,
`generate_next_sem_id` and `forward` do not build or touch it.
"""
from typing import List, NamedTuple, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from data.schemas import TokenizedSeqBatch
from modules.sid_items import SemIdItemIndex
from modules.sid_prefix import SemIdPrefixIndex
from modules.t5 import STACK_ATTRIBUTES, PackedRows, T5Config, T5EncoderModel, T5Stack, checked
from rqhip import ops
from rqhip._lib import RqHipError
from rqhip.autograd import RowsPackFunction, SidEmbedFunction, SidHeadLossFunction

HEAD_IMPLS = ("torch", "hip")
ENCODER_ROWS = ("padded", "packed")
EMBED_IMPLS = ("torch", "hip")
BEAM_IMPLS = ("sample", "exact")


class ModelOutput(NamedTuple):
    loss: Tensor
    logits: Tensor
    loss_d: Tensor


class GenerationOutput(NamedTuple):
    sem_ids: Tensor
    log_probas: Tensor


class ItemRecommendation(NamedTuple):
    items: Tensor        # [B, n_items] int64 corpus item numbers, best first, -1 padded
    scores: Tensor       # [B, n_items] fp32: the log probability of the beam each item came from, -inf padded
    sem_ids: Tensor      # [B, k, num_hierarchies] int64, as GenerationOutput
    log_probas: Tensor   # [B, k] fp32, as GenerationOutput


def _strip_dedup_col(tensor: Tensor, sem_ids_dim: int, n_layers: int) -> Tensor:
    """[B, N * sem_ids_dim] (n_layers ids + the tokenizer's dedup column per item) -> [B, N * n_layers]."""
    B, total = tensor.shape
    N = total // sem_ids_dim
    return tensor.view(B, N, sem_ids_dim)[:, :, :n_layers].contiguous().view(B, N * n_layers)


def _exponential_like(probas: Tensor) -> Tensor:
    """The Exp(1) draw of torch.multinomial without replacement, from the current device generator."""
    return torch.empty_like(probas).exponential_(1)


class EncoderDecoderRetrievalModel(nn.Module):
    def __init__(
        self,
        codebooks: Tensor,
        num_hierarchies: int,
        num_embeddings_per_hierarchy: int,
        t5_d_model: int = 128,
        t5_num_heads: int = 6,
        t5_d_ff: int = 1024,
        t5_num_layers: int = 4,
        top_k_for_generation: int = 10,
        should_add_sep_token: bool = True,
        num_user_bins: Optional[int] = None,
    ):
        super().__init__()
        self.num_hierarchies = num_hierarchies
        self.num_embeddings_per_hierarchy = num_embeddings_per_hierarchy
        self.top_k_for_generation = top_k_for_generation
        self.register_buffer("codebooks", codebooks)

        vocab = num_embeddings_per_hierarchy * num_hierarchies
        self.encoder = T5EncoderModel(T5Config(vocab, d_model=t5_d_model, num_heads=t5_num_heads, d_ff=t5_d_ff,
                                               num_layers=t5_num_layers, is_decoder=False))
        self.t5_decoder = T5Stack(T5Config(vocab, d_model=t5_d_model, num_heads=t5_num_heads, d_ff=t5_d_ff,
                                           num_layers=t5_num_layers, is_decoder=True))
        self.bos_token = nn.Parameter(torch.randn(1, t5_d_model), requires_grad=True)
        self.decoder_mlp = nn.ModuleList(
            [nn.Linear(t5_d_model, num_embeddings_per_hierarchy, bias=False) for _ in range(num_hierarchies)])
        # one table for all hierarchies: level h, code t -> row h * codebook_size + t
        self.item_sid_embedding_table = nn.Embedding(num_embeddings=vocab, embedding_dim=t5_d_model)
        self.user_embedding = nn.Embedding(num_user_bins, t5_d_model) if num_user_bins else None
        self.sep_token = (nn.Parameter(torch.randn(1, t5_d_model), requires_grad=True)
                          if should_add_sep_token else None)

        self._prefix_index: Optional[SemIdPrefixIndex] = None
        self._prefix_key = None
        self._item_index: Optional[SemIdItemIndex] = None
        self._item_key = None
        self.attention_impl = "torch"  # or "hip" / "hip_train"; handed to both T5 stacks whenever they are run
        self.attention_long_impl = "torch"  # or "hip" (modules/t5.py); handed to both T5 stacks with attention_impl
        self.norm_impl = "torch"  # or "hip" (modules/t5.py); handed to both T5 stacks with attention_impl
        self.head_impl = "torch"  # or "hip": the heads and their losses of `forward` as one fused call
        self.ffn_impl = "torch"  # or "hip" (modules/t5.py); handed to both T5 stacks with attention_impl
        self.embed_impl = "torch"  # or "hip": each stack's input embedding as one fused call
        self.proj_impl = "torch"  # or "hip" (modules/t5.py); handed to both T5 stacks with attention_impl
        self.matmul_arith = "fp32"  # or "bf16" (modules/t5.py); handed to both T5 stacks with attention_impl
        self.attention_arith = "fp32"  # or "bf16" (modules/t5.py); handed to both T5 stacks with attention_impl
        self.weight_images = "none"  # or "bf16" (modules/t5.py); handed to both T5 stacks with attention_impl
        self.saved_activations = "fp32"  # or "bf16" (modules/t5.py); handed to both T5 stacks with attention_impl
        self.beam_impl = "sample"  # or "exact": the search of `generate` (module docstring)
        self.encoder_rows = "padded"  # or "packed": `forward` runs the encoder on the valid tokens only (module docstring)

    @property
    def device(self) -> torch.device:
        return next(self.parameters()).device

    def _add_repeating_offset_to_rows(self, input_sids: Tensor, codebook_size: int, num_hierarchies: int,
                                      attention_mask: Optional[Tensor] = None) -> Tensor:
        """Add per-hierarchy offsets so a single embedding table covers all hierarchies (times the mask: the
        tokenizer's -1 padding becomes row 0)."""
        if input_sids.ndim != 2:
            raise ValueError("Input tensor must be 2-dimensional.")
        num_cols = input_sids.shape[1]
        offsets = torch.arange(num_hierarchies, device=input_sids.device) * codebook_size
        num_repeats = (num_cols + num_hierarchies - 1) // num_hierarchies
        result = input_sids + offsets.repeat(num_repeats)[:num_cols]
        if attention_mask is not None:
            result = result * attention_mask
        return result

    def _inject_sep_token_between_sids(self, id_embeddings: Tensor, attention_mask: Tensor, sep_token: Tensor,
                                       num_hierarchies: int):
        """Append the separator embedding after each item's group of ids (the mask copies the item's last column)."""
        batch_size, seq_len, emb_dim = id_embeddings.size()
        item_count = seq_len // num_hierarchies
        emb = id_embeddings.view(batch_size, item_count, num_hierarchies, -1)
        mask = attention_mask.view(batch_size, item_count, num_hierarchies)
        sep = sep_token.unsqueeze(0).expand(batch_size, item_count, -1).unsqueeze(-2)
        id_embeddings = torch.cat([emb, sep], dim=-2)
        attention_mask = torch.cat([mask, mask[:, :, -1:]], dim=-1)  # a slice, not a host index: capturable
        return id_embeddings.reshape(batch_size, -1, emb_dim), attention_mask.reshape(batch_size, -1)

    def _prefix_index_for_codebooks(self) -> SemIdPrefixIndex:
        """The corpus' prefix index, built on first use on a device and rebuilt whenever the `codebooks` buffer
        changes (load_state_dict copies into it and bumps its version; .to() replaces it)."""
        cb = self.codebooks
        key = (cb.data_ptr(), cb.device, cb._version, tuple(cb.shape))
        if self._prefix_index is None or self._prefix_key != key:
            self._prefix_index = SemIdPrefixIndex(cb)
            self._prefix_key = key
        return self._prefix_index

    def _item_index_for_codebooks(self) -> SemIdItemIndex:
        """The corpus' (tuple, dedup rank) -> item index, cached by the rule of `_prefix_index_for_codebooks`."""
        cb = self.codebooks
        key = (cb.data_ptr(), cb.device, cb._version, tuple(cb.shape))
        if self._item_index is None or self._item_key != key:
            self._item_index = SemIdItemIndex(cb)
            self._item_key = key
        return self._item_index

    def _check_valid_prefix(self, prefix: Tensor, batch_size: int = 100000) -> Tensor:
        """Boolean mask: which rows of prefix [P, h] occur as the first h ids of a corpus row."""
        if prefix.device != self.codebooks.device:
            self.codebooks = self.codebooks.to(prefix.device)
        return self._prefix_index_for_codebooks().check_valid_prefix(prefix, batch_size)

    def _push_attention_impl(self) -> None:
        """Hand the model's stack attributes (modules/t5.py: STACK_ATTRIBUTES), validated, to both stacks."""
        for name in STACK_ATTRIBUTES:
            value = checked(self, name)
            for stack in (self.encoder.encoder, self.t5_decoder):
                setattr(stack, name, value)

    def hip_embed_active(self, input_ids: Tensor, attention_mask: Optional[Tensor] = None) -> bool:
        """Whether the "hip" input embedding is taken for these ids and this mask (module docstring)."""
        if self.embed_impl not in EMBED_IMPLS:
            raise ValueError(f"embed_impl must be one of {EMBED_IMPLS}, got {self.embed_impl!r}")
        params = [self.item_sid_embedding_table.weight, self.bos_token, self.sep_token,
                  None if self.user_embedding is None else self.user_embedding.weight]
        return (self.embed_impl == "hip" and input_ids.is_cuda and input_ids.dtype == torch.int64
                and (attention_mask is None or (attention_mask.is_cuda
                                                and attention_mask.dtype in (torch.bool, torch.int64)))
                and all(p is None or (p.is_cuda and p.dtype == torch.float32) for p in params)
                and ops.sid_embed_supported(torch.float32, self.item_sid_embedding_table.embedding_dim,
                                            self.num_hierarchies))

    def _hip_embed(self, ids, mask, ld_item, sep, prefix_table, prefix_idx, need_mask):
        """One fused call -> (inputs_embeds, its bool keep-mask or None)."""
        table = self.item_sid_embedding_table.weight
        if torch.is_grad_enabled():
            return SidEmbedFunction.apply(ids, mask, table, sep, prefix_table, prefix_idx, self.num_hierarchies, ld_item,
                                          need_mask)
        return ops.sid_embed_fwd(ids, mask, table, self.num_hierarchies, ld_item, sep, prefix_table, prefix_idx,
                                 need_mask=need_mask)

    def packed_rows_plan(self, counts: Optional[Tensor], input_ids: Tensor, with_user: bool, *, ld_item: int,
                         query_length: int) -> Optional[PackedRows]:
        """The packed form of an encoder pass over input_ids [B, S * ld_item] (module docstring, `encoder_rows`), or None:
        the padded path.  `forward` asks with the batch's item_counts, its sem_ids as they are (ld_item = L + 1) and the
        decoder's query length L + 1; `generate` with its own arguments (ld_item = L) and the decode step's query length
        1.  with_user: the caller passes user ids.  Built on the host from `counts` and the shapes alone; the only
        device work is the upload of the cumulative table."""
        if self.encoder_rows not in ENCODER_ROWS:
            raise ValueError(f"encoder_rows must be one of {ENCODER_ROWS}, got {self.encoder_rows!r}")
        if self.encoder_rows != "packed" or counts is None or not input_ids.is_cuda:
            return None
        B, L = input_ids.shape[0], self.num_hierarchies
        S = input_ids.shape[1] // ld_item
        if counts.is_cuda or counts.dtype != torch.int64 or tuple(counts.shape) != (B,):
            raise ValueError(f"item_counts must be an int64 CPU tensor [{B}], got {counts.dtype} {tuple(counts.shape)} "
                             f"on {counts.device}")
        if B == 0 or int(counts.min()) < 0 or int(counts.max()) > S:
            return None
        with_user = with_user and self.user_embedding is not None
        if not with_user and int(counts.min()) == 0:
            return None   # a row without a token: its padded form attends uniformly over its padding
        per_item = L + (1 if self.sep_token is not None else 0)
        bound = int(with_user) + S * per_item
        table = self.item_sid_embedding_table.weight
        self._push_attention_impl()
        if not (ops.rows_pack_supported(table.dtype, table.shape[1])
                and self.encoder.encoder.packed_rows_active(table, bound, bound)
                and self.t5_decoder.packed_rows_active(table, query_length, bound)):
            return None
        cu = torch.zeros(B + 1, dtype=torch.int32)
        cu[1:] = torch.cumsum(int(with_user) + counts * per_item, 0)
        return PackedRows(cu.pin_memory().to(table.device, non_blocking=True), bound, B, int(cu[-1]))

    def _encode(self, inputs_embeds: Tensor, attention_mask, rows: Optional[PackedRows]):
        """The encoder on the front's output -> (encoder output, its keep-mask); with `rows` on the valid tokens only:
        one pack launch, then the stack on [1, N, d], whose output needs no mask."""
        if rows is None:
            return self.encoder(inputs_embeds=inputs_embeds, attention_mask=attention_mask), attention_mask
        if torch.is_grad_enabled():
            packed = RowsPackFunction.apply(inputs_embeds, rows.cu, rows.rows)
        else:
            packed = ops.rows_pack(inputs_embeds, rows.cu, rows.rows)
        return self.encoder.encoder(packed.unsqueeze(0), packed=rows), None

    def encoder_forward_pass(self, attention_mask, input_ids, user_id=None, *, ld_item=None,
                             rows: Optional[PackedRows] = None):
        """ld_item: columns per item in input_ids and attention_mask, num_hierarchies (the default) or more; columns
        past num_hierarchies of an item (the tokenizer's dedup column) are not read.  rows (`packed_rows_plan`): the
        encoder runs on the valid tokens only and the result is ([1, N, d], None)."""
        self._push_attention_impl()
        ld_item = self.num_hierarchies if ld_item is None else ld_item
        with_user = user_id is not None and self.user_embedding is not None
        if attention_mask is not None and self.hip_embed_active(input_ids, attention_mask):
            inputs_embeds, attention_mask = self._hip_embed(
                input_ids, attention_mask, ld_item, self.sep_token,
                self.user_embedding.weight if with_user else None, user_id if with_user else None, True)
            return self._encode(inputs_embeds, attention_mask, rows)
        if ld_item != self.num_hierarchies:
            input_ids = _strip_dedup_col(input_ids, ld_item, self.num_hierarchies)
            attention_mask = _strip_dedup_col(attention_mask.long(), ld_item, self.num_hierarchies)
        shifted = self._add_repeating_offset_to_rows(input_sids=input_ids,
                                                     codebook_size=self.num_embeddings_per_hierarchy,
                                                     num_hierarchies=self.num_hierarchies,
                                                     attention_mask=attention_mask)
        inputs_embeds = self.item_sid_embedding_table(shifted)
        if self.sep_token is not None:
            inputs_embeds, attention_mask = self._inject_sep_token_between_sids(
                id_embeddings=inputs_embeds, attention_mask=attention_mask, sep_token=self.sep_token,
                num_hierarchies=self.num_hierarchies)
        if with_user:
            user_embeds = self.user_embedding(torch.remainder(user_id[:, 0], self.user_embedding.num_embeddings))
            inputs_embeds = torch.cat([user_embeds.unsqueeze(1), inputs_embeds], dim=1)
            attention_mask = torch.cat(
                [torch.ones(attention_mask.size(0), 1, device=attention_mask.device), attention_mask], dim=1)
        return self._encode(inputs_embeds, attention_mask, rows)

    def decoder_forward_pass(self, attention_mask=None, future_ids=None, encoder_output=None,
                             attention_mask_for_encoder=None, use_cache=False, past_key_values=None, *, ld_item=None,
                             encoder_rows: Optional[PackedRows] = None):
        """encoder_rows: encoder_output is the packed [1, N, d] of `encoder_forward_pass(rows=...)`.
        BOS followed by the embedded future ids (or BOS alone); with a cache (the list this returns when use_cache)
        only the last future id is run.  Returns the hidden states, and the self-attention cache when use_cache.
        ld_item: as in encoder_forward_pass, for future_ids and attention_mask."""
        self._push_attention_impl()
        ld_item = self.num_hierarchies if ld_item is None else ld_item
        if (future_ids is not None and not past_key_values and future_ids.dim() == 2
                and future_ids.shape[1] >= ld_item and future_ids.shape[1] % ld_item == 0
                and self.hip_embed_active(future_ids, attention_mask)):
            inputs_embeds, attention_mask = self._hip_embed(future_ids, attention_mask, ld_item, None, self.bos_token,
                                                            None, attention_mask is not None)
        elif future_ids is not None:
            if ld_item != self.num_hierarchies:
                future_ids = _strip_dedup_col(future_ids, ld_item, self.num_hierarchies)
                if attention_mask is not None:
                    attention_mask = _strip_dedup_col(attention_mask, ld_item, self.num_hierarchies)
            shifted = self._add_repeating_offset_to_rows(
                input_sids=future_ids, codebook_size=self.num_embeddings_per_hierarchy,
                num_hierarchies=self.num_hierarchies,
                attention_mask=torch.ones_like(future_ids) if attention_mask is None else attention_mask)
            inputs_embeds = self.item_sid_embedding_table(shifted)
            if not past_key_values:
                bos = self.bos_token.unsqueeze(0).expand(future_ids.size(0), 1, -1)
                inputs_embeds = torch.cat([bos, inputs_embeds], dim=1)
                if attention_mask is not None:
                    attention_mask = torch.cat(
                        [torch.ones(future_ids.size(0), 1, device=future_ids.device), attention_mask], dim=1)
            else:
                inputs_embeds = inputs_embeds[:, -1:, :]
        else:
            inputs_embeds = self.bos_token.unsqueeze(0).expand(encoder_output.size(0), 1, -1)
        return self.t5_decoder(inputs_embeds, attention_mask=attention_mask, encoder_hidden_states=encoder_output,
                               encoder_attention_mask=attention_mask_for_encoder,
                               past_key_values=past_key_values or None, use_cache=use_cache,
                               encoder_packed=encoder_rows)

    def hip_head_active(self, decoder_output: Tensor) -> bool:
        """Whether `forward` takes the "hip" head path for this decoder output (module docstring)."""
        if self.head_impl not in HEAD_IMPLS:
            raise ValueError(f"head_impl must be one of {HEAD_IMPLS}, got {self.head_impl!r}")
        return (self.head_impl == "hip" and decoder_output.is_cuda
                and all(m.weight.dtype == decoder_output.dtype for m in self.decoder_mlp)
                and ops.sid_head_loss_supported(decoder_output.dtype, decoder_output.shape[-1],
                                                self.num_embeddings_per_hierarchy, self.num_hierarchies))

    def forward(self, batch: TokenizedSeqBatch) -> ModelOutput:
        sem_ids_dim = self.num_hierarchies + 1
        fut_ids = batch.sem_ids_fut[:, : self.num_hierarchies]
        rows = self.packed_rows_plan(getattr(batch, "item_counts", None), batch.sem_ids, batch.user_ids is not None,
                                     ld_item=sem_ids_dim, query_length=sem_ids_dim)   # None: the padded path (the default)
        if self.hip_embed_active(batch.sem_ids, batch.seq_mask):      # the batch's tensors as they are
            encoder_output, attention_mask_for_encoder = self.encoder_forward_pass(
                attention_mask=batch.seq_mask, input_ids=batch.sem_ids, user_id=batch.user_ids, ld_item=sem_ids_dim,
                rows=rows)
            decoder_output = self.decoder_forward_pass(
                future_ids=batch.sem_ids_fut, encoder_output=encoder_output,
                attention_mask_for_encoder=attention_mask_for_encoder, use_cache=False, ld_item=sem_ids_dim,
                encoder_rows=rows)
        else:
            input_ids = _strip_dedup_col(batch.sem_ids, sem_ids_dim, self.num_hierarchies)
            attention_mask = _strip_dedup_col(batch.seq_mask.long(), sem_ids_dim, self.num_hierarchies)
            encoder_output, attention_mask_for_encoder = self.encoder_forward_pass(
                attention_mask=attention_mask, input_ids=input_ids, user_id=batch.user_ids, rows=rows)
            decoder_output = self.decoder_forward_pass(
                future_ids=fut_ids, encoder_output=encoder_output,
                attention_mask_for_encoder=attention_mask_for_encoder, use_cache=False, encoder_rows=rows)
        if self.hip_head_active(decoder_output):
            weights = [m.weight for m in self.decoder_mlp]
            if torch.is_grad_enabled():
                loss, loss_d = SidHeadLossFunction.apply(decoder_output, batch.sem_ids_fut, *weights)
            else:
                loss, loss_d = ops.sid_head_loss_fwd(decoder_output, weights, batch.sem_ids_fut, self.num_hierarchies)[:2]
            return ModelOutput(loss=loss, logits=None, loss_d=loss_d)
        decoder_output = decoder_output[:, :-1]
        total_loss = torch.tensor(0.0, device=decoder_output.device)
        loss_d = []
        for h in range(self.num_hierarchies):
            logits = self.decoder_mlp[h](decoder_output[:, h])
            h_loss = F.cross_entropy(logits, fut_ids[:, h].long())
            total_loss = total_loss + h_loss
            loss_d.append(h_loss.detach())
        return ModelOutput(loss=total_loss, logits=None, loss_d=torch.stack(loss_d))

    @torch.no_grad()
    def generate(self, attention_mask, input_ids, user_id=None, *, item_counts=None):
        """Beam search over the hierarchy levels: the reference's sampling search (beam_impl = "sample"), or the exact
        constrained search (beam_impl = "exact", module docstring), which replaces the noise draw and ops.beam_step below
        by one ops.beam_topk_step over all K codes per beam and needs k <= K.

        Step 0 decodes BOS on the B users and keeps the best k of n_cands = min(64, K) samples; every later step runs
        the B * k beams' newest id through the decoder (self-attention cache reordered by parent beam; cross-attention
        K/V computed once on the B users) and one ops.beam_step.  With attention_impl = "hip" the self-attention cache
        is a T5DecodeCache instead: each step's K/V are projected straight into that position's slab and the parent
        beams reorder a small ancestor table, never the K/V.

        item_counts (int64 CPU [B], the leading valid item slots of each row of input_ids; a CountedSeqBatch's) with
        encoder_rows = "packed": the encoder, the cross K/V and every decode step's cross-attention run on the valid
        tokens only (`packed_rows_plan`; module docstring), with the padded run's bits.  Such a call cannot be captured
        into a graph: its row count N depends on the data.  Without counts, or wherever the packed form does not apply,
        the padded path runs, silently.

        Returns generated_ids [B, k, num_hierarchies] int64 and log_probas [B, k] fp32 (-inf for beams without a valid
        corpus prefix)."""
        k = self.top_k_for_generation
        n_cands = min(64, self.num_embeddings_per_hierarchy)
        if self.beam_impl not in BEAM_IMPLS:
            raise ValueError(f"beam_impl must be one of {BEAM_IMPLS}, got {self.beam_impl!r}")
        exact = self.beam_impl == "exact"
        if exact and k > self.num_embeddings_per_hierarchy:
            raise ValueError(f"top_k_for_generation={k} exceeds the K={self.num_embeddings_per_hierarchy} codes of the "
                             f"first step (num_embeddings_per_hierarchy)")
        if not exact and k > n_cands:
            raise ValueError(f"top_k_for_generation={k} exceeds the n_cands={n_cands} samples of the first step "
                             f"(min(64, num_embeddings_per_hierarchy))")
        if not self.codebooks.is_cuda or not input_ids.is_cuda:
            raise RqHipError("generate needs ROCm device tensors: the beam step is a HIP kernel with no CPU path")
        if input_ids.device != self.codebooks.device:
            self.codebooks = self.codebooks.to(input_ids.device)
        index = self._prefix_index_for_codebooks()
        index.to(input_ids.device)

        dec = self.t5_decoder
        rows = self.packed_rows_plan(item_counts, input_ids, user_id is not None, ld_item=self.num_hierarchies,
                                     query_length=1)
        if rows is not None and not dec.hip_attention_active(self.item_sid_embedding_table.weight, 1,
                                                             self.num_hierarchies, rows.bound, cached=True):
            rows = None   # the packed decode step lives on the slabs: without them the padded path
        enc_out, enc_mask = self.encoder_forward_pass(attention_mask=attention_mask, input_ids=input_ids,
                                                      user_id=user_id, rows=rows)   # packed: ([1, N, d], None)
        cross_kv = dec.cross_kv(enc_out)
        B = input_ids.shape[0]
        cross_length = enc_out.shape[1] if rows is None else rows.bound
        K = self.num_embeddings_per_hierarchy

        x = self.bos_token.unsqueeze(0).expand(B, 1, -1)
        self_kv: Optional[List] = None
        slabs = None
        if dec.hip_attention_active(enc_out, 1, self.num_hierarchies, cross_length, cached=True):
            slabs = dec.new_decode_cache(self.num_hierarchies, B * k, enc_out.device)
        ids = scores = None
        for h in range(self.num_hierarchies):
            if h > 0:
                x = self.item_sid_embedding_table(ids[:, :, h - 1].reshape(-1, 1) + (h - 1) * K)
            if slabs is not None:
                if h > 0:
                    slabs.reorder(parent)
                hidden = dec(x, encoder_attention_mask=enc_mask, cross_kv=cross_kv, decode_cache=slabs,
                             encoder_packed=rows)
            else:
                if h > 0:
                    rows = parent.flatten()
                    self_kv = [(kk.index_select(0, rows), vv.index_select(0, rows)) for kk, vv in self_kv]
                hidden, self_kv = dec(x, encoder_attention_mask=enc_mask, past_key_values=self_kv, use_cache=True,
                                      cross_kv=cross_kv)
            logits = F.linear(hidden[:, -1], self.decoder_mlp[h].weight)
            if exact:
                ids, scores, parent = ops.beam_topk_step(logits, scores, ids, index._index, index._corpus, k)
            else:
                noise = _exponential_like(logits)
                ids, scores, parent = ops.beam_step(logits, noise, scores, ids, index._index, index._corpus, n_cands, k)
        return ids, scores

    @torch.no_grad()
    def generate_next_sem_id(self, batch: TokenizedSeqBatch, top_k: bool = True,
                             temperature: int = 1) -> GenerationOutput:
        sem_ids_dim = self.num_hierarchies + 1
        input_ids = _strip_dedup_col(batch.sem_ids, sem_ids_dim, self.num_hierarchies)
        attention_mask = _strip_dedup_col(batch.seq_mask.long(), sem_ids_dim, self.num_hierarchies)
        generated_ids, log_probas = self.generate(attention_mask=attention_mask, input_ids=input_ids,
                                                  user_id=batch.user_ids, item_counts=getattr(batch, "item_counts", None))
        return GenerationOutput(sem_ids=generated_ids, log_probas=log_probas)

    @torch.no_grad()
    def recommend_items(self, batch: TokenizedSeqBatch, n_items: Optional[int] = None,
                        exclude_history: bool = True) -> ItemRecommendation:
        """The items to recommend to each user of the batch: one `generate_next_sem_id(batch)` call and ONE launch that
        expands its beams to corpus item numbers (SemIdItemIndex.expand; the semantics are in include/rqhip.h).

        n_items defaults to top_k_for_generation (at most 256).  With exclude_history the items of batch.sem_ids -- the
        batch's tensor as it is, dedup column included, negative ids being padding -- are never returned.  A user gets
        fewer than n_items items (-1 / -inf padded) when the finite beams' tuples carry fewer.  After the encoder nothing
        is read back to the host and no allocation depends on data, as in `generate` -- whose packed form (a
        CountedSeqBatch under encoder_rows = "packed") this call takes too, with the same items and scores."""
        n_items = self.top_k_for_generation if n_items is None else int(n_items)
        generated = self.generate_next_sem_id(batch)
        index = self._item_index_for_codebooks()   # `generate` has moved `codebooks` to the batch's device
        index.to(generated.sem_ids.device)
        items, scores = index.expand(generated.sem_ids, generated.log_probas, n_items,
                                     history=batch.sem_ids if exclude_history else None)
        return ItemRecommendation(items=items, scores=scores, sem_ids=generated.sem_ids,
                                  log_probas=generated.log_probas)
