"""From generated semantic-id tuples to corpus items.

The retrieval model generates L-tuples of semantic ids, but several corpus items can share a tuple: the tokenizer tells
them apart by a dedup column, "how many earlier items have the same tuple" (`SemanticIdTokenizer.precompute_corpus_ids`,
modules/tokenizer/semids.py), which the decoder never generates.  `SemIdItemIndex` is the inverse of the tokenizer's
lookup: an exact map (tuple, dedup rank) -> item number, built once per corpus on the device (csrc/sid_items.hip), and
the one-launch expansion of a `generate` result into the item numbers a recommender returns.

    index = SemIdItemIndex(codebooks)                 # codebooks [N, L] int64, the model's buffer
    item = index.items_of(ids)                        # ids [P, L + 1] (tuple, dedup rank) -> int64 [P], -1 = no such item
    items, scores = index.expand(beams, log_probas, n, history=batch.sem_ids)

`expand` walks a user's beams best first and gives each beam's items in ascending item number, without the items of the
user's history (rows of `history`, in the form of batch.sem_ids, dedup column included; negative ids are padding), cut
at n; the exact semantics are in include/rqhip.h.  The dedup ranks are computed here with ops.dedup_rank, the
tokenizer's own law, so they equal tokenizer.cached_ids[:, L].

Replicated per rank like the prefix index (12 to 20 bytes per item); there is no CPU path.
"""
from typing import Optional, Tuple

import torch
from torch import Tensor

from rqhip import ops


class SemIdItemIndex:
    def __init__(self, codebooks: Tensor) -> None:
        if codebooks.dim() != 2 or codebooks.dtype != torch.int64:
            raise ValueError(f"codebooks must be an int64 [N, n_layers] tensor, got {codebooks.dtype} "
                             f"{tuple(codebooks.shape)}")
        self.codebooks = codebooks
        self._index = None
        if codebooks.is_cuda:
            self._build()

    def _build(self) -> None:
        # private dense copy: the index stores row numbers of exactly this tensor
        self._corpus = self.codebooks.detach().contiguous().clone()
        self.ranks, _ = ops.dedup_rank(self._corpus.t().contiguous())
        self._index = ops.sid_item_index_build(self._corpus, self.ranks)

    def to(self, device) -> "SemIdItemIndex":
        device = torch.device(device)
        if self.codebooks.device != device:
            self.codebooks = self.codebooks.to(device)
            self._index = None
        if self._index is None and self.codebooks.is_cuda:
            self._build()
        return self

    @property
    def num_items(self) -> int:
        return self.codebooks.shape[0]

    def _ready(self, like: Tensor) -> None:
        if like.device != self.codebooks.device:
            self.to(like.device)
        if self._index is None:
            self._build()  # on a CPU tensor this raises RqHipError: there is no CPU implementation

    @torch.no_grad()
    def items_of(self, ids: Tensor) -> Tensor:
        """ids [P, L + 1] int64, tuple and dedup rank (a row of tokenizer.cached_ids or of batch.sem_ids_fut) -> the item
        numbers, int64 [P]; -1 where no corpus item has that tuple and rank."""
        self._ready(ids)
        return ops.sid_item_lookup(self._index, self._corpus, ids)

    @torch.no_grad()
    def expand(self, beams: Tensor, scores: Tensor, n: int, history: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        """beams [B, k, L] int64 and scores [B, k] fp32 as `generate` returns them -> items [B, n] int64 (-1 padded) and
        their beams' scores [B, n] fp32 (-inf padded), in one launch."""
        self._ready(beams)
        return ops.sid_items_topn(self._index, self._corpus, beams, scores, n, history)
