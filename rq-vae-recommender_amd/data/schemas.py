"""Batch containers exchanged between the data layer, RqVae and the tokenizer.

Field names and order follow reference data/schemas.py:7-22 because callers construct and unpack these
positionally (`SeqBatch(*[...])` in data/utils.py, `batch.x` in modules/rqvae.py)."""
import collections

FUT_SUFFIX = "_fut"

#: one batch of items or user sequences; RqVae.forward reads only `.x` (reference modules/rqvae.py:143)
SeqBatch = collections.namedtuple("SeqBatch", ["user_ids", "ids", "ids" + FUT_SUFFIX, "x", "x" + FUT_SUFFIX, "seq_mask"])

#: output of SemanticIdTokenizer.forward (reference modules/tokenizer/semids.py:139-146)
TokenizedSeqBatch = collections.namedtuple(
    "TokenizedSeqBatch",
    ["user_ids", "sem_ids", "sem_ids" + FUT_SUFFIX, "seq_mask", "token_type_ids", "token_type_ids" + FUT_SUFFIX],
)


class CountedSeqBatch(TokenizedSeqBatch):
    """A TokenizedSeqBatch -- the same six fields, `_fields` and positional unpacking -- that also says, on the HOST, how
    many history items each row holds: `item_counts`, an int64 CPU tensor [B], the number of leading valid item slots of
    seq_mask's rows.  data/seq_loader.py yields it with host_windows=True; modules/model.py reads it to run the encoder
    on the valid tokens only (encoder_rows = "packed") without reading the device."""

    def __new__(cls, *args, item_counts=None, **kwargs):
        self = super().__new__(cls, *args, **kwargs)
        self.item_counts = item_counts
        return self

    def _replace(self, **kwargs):
        out = super()._replace(**kwargs)
        out.item_counts = self.item_counts
        return out
