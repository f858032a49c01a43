"""Tokenized training batches of the retrieval model straight from device-resident histories.

The reference feeds its loop with `DataLoader(SeqData, batch_size, shuffle=True)`: one Python `__getitem__` per user,
a collate, a host-to-device copy and `SemanticIdTokenizer.forward` on the result.  What the model consumes is a pure
function of the stored histories, the tokenizer's cached id table and two random integers per row, so
`TokenizedSeqLoader` builds it where it is used: per epoch one `torch.randperm` on the device (an `arange` without
shuffling), per batch one `torch.randint` (training rows only) and one kernel launch
(SemanticIdTokenizer.tokenize_rows -> ops.seq_batch, csrc/seq_batch.hip).  Nothing is read back by the host and no
allocation has a size that depends on data, so the calls of a batch can be recorded into a graph (not done here).

Batches are `DataLoader`'s default: every user once per epoch, the short last batch kept, `len(loader)` =
ceil(U / batch_size).  The constant token_type_ids are written once per batch size and shared by every later batch of
that size; they are never written to.

`host_windows=True` (default False: the loader above, bit for bit, with the same RNG use) draws the permutation and the
two integers per row from torch's CPU generator instead (`torch.manual_seed` reproduces an epoch) and uploads them; the
same one launch builds the batch.  The host then knows each row's window: a vectorised restatement of `seq_window`
(data/processed.py:seq_window_counts) on the host copy of the history lengths gives the rows' item counts, and the batch
is a `CountedSeqBatch` carrying them as `item_counts` (int64 CPU [B]).  That is what lets the model run the encoder on
the valid tokens only (modules/model.py: encoder_rows = "packed") with a row count the host never has to read back."""
import torch

from data.processed import SeqData, seq_window_counts
from data.schemas import CountedSeqBatch, TokenizedSeqBatch


def _upload(t: torch.Tensor, device) -> torch.Tensor:
    """A small host tensor to the device without making the host wait for the device."""
    if torch.device(device).type != "cuda":
        return t.to(device)
    return t.pin_memory().to(device, non_blocking=True)


class TokenizedSeqLoader:
    def __init__(self, seq_data: SeqData, tokenizer, batch_size: int, shuffle: bool = True,
                 host_windows: bool = False) -> None:
        if batch_size < 1:
            raise ValueError(f"batch_size must be positive, got {batch_size}")
        if tokenizer.cached_ids is None:
            raise RuntimeError("TokenizedSeqLoader needs the corpus ids: call tokenizer.precompute_corpus_ids first")
        seq_data.check_items(len(tokenizer.cached_ids))       # once, on the host: no per-batch range test is needed
        self.seq_data, self.tokenizer, self.batch_size, self.shuffle = seq_data, tokenizer, int(batch_size), shuffle
        self._token_types = {}                                  # rows of a batch -> (token_type_ids, token_type_ids_fut)
        self.host_windows = bool(host_windows)

    def __len__(self) -> int:
        return -(-len(self.seq_data) // self.batch_size)

    def __iter__(self):
        U, dev = len(self.seq_data), self.seq_data.offsets.device
        if self.host_windows:
            yield from self._iter_host(U, dev)
            return
        perm = torch.randperm(U, device=dev) if self.shuffle else torch.arange(U, device=dev)
        for start in range(0, U, self.batch_size):
            yield self._batch(perm[start:start + self.batch_size])

    def _iter_host(self, U: int, dev):
        """An epoch with the permutation and the draws made on the host (module docstring)."""
        data = self.seq_data
        perm = torch.randperm(U) if self.shuffle else torch.arange(U)
        for start in range(0, U, self.batch_size):
            rows = perm[start:start + self.batch_size]
            draws = (torch.randint(0, 2 ** 62, (rows.shape[0], 2), dtype=torch.int64) if data.subsample else None)
            counts = seq_window_counts(data.host_lengths[rows], draws, data.max_seq_len, data.subsample)
            batch = self._batch(_upload(rows, dev), None if draws is None else _upload(draws, dev))
            yield CountedSeqBatch(*batch, item_counts=counts)

    def _batch(self, rows: torch.Tensor, draws=None) -> TokenizedSeqBatch:
        cached = self._token_types.get(rows.shape[0])
        batch = self.tokenizer.tokenize_rows(self.seq_data, rows, draws=draws, token_types=cached is None)
        if cached is None:
            self._token_types[rows.shape[0]] = (batch.token_type_ids, batch.token_type_ids_fut)
            return batch
        return batch._replace(token_type_ids=cached[0], token_type_ids_fut=cached[1])
