"""Item-feature dataset for RQ-VAE training: an HBM-resident stand-in for the reference's `ItemData`.

The reference's data layer (data/processed.py:39-86 on top of data/amazon.py, data/ml32m.py, ...) downloads
raw datasets and embeds item text with sentence-T5-XXL through torch_geometric / polars -- out of scope for
this repo and impossible offline.  What the hot path needs from it is small and is kept
verbatim: `len(ds)` and `ds[idx] -> SeqBatch` with `x = item_matrix[idx, :768]` for an int / list / tensor
index (processed.py:74-86), train/eval/all splits driven by an `is_train` mask, and the `RecDataset` enum
that gin configs name as `%data.processed.RecDataset.AMAZON`.

Source of the matrix, in order:
  1. `<root>/item_features.pt` -- a dict {"x": float32 [N, >=768], "is_train": bool [N] (optional)} that a
     user exports once from the reference's processed HeteroData (`data["item"].x`, `["is_train"]`);
  2. ONLY when the folder is NAMED "synthetic:<N>" (e.g. `train.dataset_folder="synthetic:87585"`: an explicit opt-in
     in the configuration itself, loud warning, `ds.synthetic` is True): a deterministic synthetic corpus of N unit-norm
     768-d rows (seed 1234) with the reference's 95/5 split (seed 42, data/amazon.py:154-156).  Otherwise a missing file
     raises FileNotFoundError -- the reference would download the data or fail here, never train on noise.
MI355X-first: the matrix is moved to the GPU once (`to_device`) and batches are gathered there -- 10 M x 768
fp32 = 30.7 GB fits one 288 GB HBM stack many times over -- so no PCIe copy sits in the training loop.

`SeqData` (below) is the stand-in for the reference's user-sequence dataset of the retrieval model (processed.py:89-169):
same constructor and `ds[i]`, histories held unpadded in CSR form from `<root>/sequences.pt` or the same explicit
synthetic opt-in, resident on the device for data/seq_loader.py; `seq_window` is the law of a training row.
"""
import os
from enum import Enum
from typing import Optional

import torch
from torch import Tensor
from torch.utils.data import Dataset

from data.schemas import SeqBatch

try:
    import gin
except ImportError:  # pragma: no cover
    from rqhip import ginlite as gin

FEATURE_DIM = 768


@gin.constants_from_enum
class RecDataset(Enum):
    AMAZON = 1
    ML_1M = 2
    ML_32M = 3


def synthetic_item_matrix(n_items: int, dim: int = FEATURE_DIM, seed: int = 1234) -> Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n_items, dim, generator=g), dim=-1)


def synthetic_train_mask(n_items: int, seed: int = 42, p_train: float = 0.95) -> Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n_items, generator=g) > (1.0 - p_train)


class ItemData(Dataset):
    def __init__(self, root: str, *args, force_process: bool = False, dataset: RecDataset = RecDataset.ML_1M,
                 train_test_split: str = "all", item_matrix: Optional[Tensor] = None,
                 is_train: Optional[Tensor] = None, **kwargs) -> None:
        del args, kwargs, force_process  # accepted for signature compatibility (split=..., etc.)
        self.dataset = dataset
        self.synthetic = False
        if item_matrix is None:
            path = os.path.join(root, "item_features.pt")
            if str(root).startswith("synthetic:"):
                # explicit opt-in only, spelled out in the configuration: a run on noise must never look like a run on
                # the dataset
                n = int(str(root).split(":", 1)[1])
                print(f"[ItemData] WARNING: dataset folder {root!r} -- using {n} SYNTHETIC unit-norm items; "
                      "results say nothing about a real corpus", flush=True)
                item_matrix = synthetic_item_matrix(n)
                self.synthetic = True
            elif os.path.exists(path):
                blob = torch.load(path, map_location="cpu", weights_only=True)
                item_matrix, is_train = blob["x"].to(torch.float32), blob.get("is_train", is_train)
            else:
                raise FileNotFoundError(
                    f"{path} not found.  Export the item features first (INTEGRATION.md, 'Item features': "
                    "torch.save({'x': item_matrix_fp32[N, >=768], 'is_train': mask}, '<dataset_folder>/item_features.pt')) "
                    "or opt in to synthetic items explicitly by naming the folder 'synthetic:<n>'.")
        if is_train is None:
            is_train = synthetic_train_mask(item_matrix.shape[0])
        if train_test_split == "train":
            keep = is_train
        elif train_test_split == "eval":
            keep = ~is_train
        elif train_test_split == "all":
            keep = None            # every row: the matrix itself, no masked copy (10 M x 768 fp32 is 30.7 GB)
        else:
            raise ValueError(f"unknown train_test_split {train_test_split!r}")
        self.item_data = item_matrix if keep is None else item_matrix[keep.to(item_matrix.device)]
        self._row_max = self._col_max = None

    def to_device(self, device) -> "ItemData":
        """Make the feature matrix resident on `device` (HBM); later `ds[idx]` gathers happen there."""
        self.item_data = self.item_data.to(device)
        self._row_max = self._col_max = None
        return self

    # batches of this many rows and more run the MLPs' fp16-split kernels, which scale every row by its largest |value|
    # (rqhip/linear.py:SPLIT_MIN_ROWS): that maximum is a property of the item, computed once per corpus and gathered with the batch
    @property
    def _SCALES_MIN_ROWS(self) -> int:
        from rqhip import linear as _lin
        return _lin.SPLIT_MIN_ROWS

    def _corpus_maxima(self):
        """(row maxima int32 [N], column maxima int32 [768]) of the resident matrix's feature columns, bit patterns (rqhip_maxima)."""
        if getattr(self, "_row_max", None) is None:
            from rqhip import ops
            x = self.item_data
            n, step = x.shape[0], 1 << 20
            rows, cols = [], None
            for lo in range(0, n, step):
                part = x[lo:lo + step, :FEATURE_DIM]
                r, c, _ = ops.maxima(part if part.is_contiguous() else part.contiguous())
                rows.append(r[0])
                cols = c if cols is None else torch.maximum(cols, c)       # (bit patterns of non-negative floats order like integers)
            self._row_max, self._col_max = torch.cat(rows), cols
        return self._row_max, self._col_max

    def __len__(self) -> int:
        return self.item_data.shape[0]

    def __getitem__(self, idx) -> SeqBatch:
        dev = self.item_data.device
        item_ids = idx.to(dev) if isinstance(idx, Tensor) else torch.tensor(idx, device=dev).unsqueeze(0)
        rows = idx.to(dev) if isinstance(idx, Tensor) else idx
        minus_one = -1 * torch.ones_like(item_ids.squeeze(0))
        x = self.item_data[rows, :FEATURE_DIM]
        if (x.is_cuda and isinstance(rows, Tensor) and rows.dim() == 1 and rows.numel() >= self._SCALES_MIN_ROWS
                and x.dtype == torch.float32 and x.shape[1] % 4 == 0):
            from rqhip import linear as _lin
            rm, cm = self._corpus_maxima()
            _lin.attach_scales(x, rm[rows].unsqueeze(0), cm)    # the rows' maxima travel with the rows; corpus-wide column bounds
        return SeqBatch(user_ids=minus_one, ids=item_ids, ids_fut=minus_one, x=x,
                        x_fut=minus_one, seq_mask=torch.ones_like(item_ids, dtype=torch.bool))


# ---- user sequences (the reference's SeqData, data/processed.py:89-169) ---------------------------------------------

MAX_SEQ_LEN = {RecDataset.AMAZON: 20, RecDataset.ML_1M: 200, RecDataset.ML_32M: 200}
SEQ_SPLITS = ("train", "eval", "test")
SEQ_FIELDS = ("userId", "offsets", "items", "itemId_fut")


def seq_window(n_hist: int, u0: int, u1: int, S: int, subsample: bool):
    """The window law of a training row -> (first, n_items, fut_pos); csrc/seq_batch.hip restates it.

    A user's sequence `seq` is the n_hist history items followed by the future item: n = n_hist + 1 elements.  The row's
    history is seq[first : first + n_items], padded at the tail to S = max_seq_len >= 2, its target is seq[fut_pos]
    (fut_pos == n_hist is the stored future item).

    subsample (the reference's training rows): start = u0 % (max(0, n - 3) + 1), end = start + 3 + u1 % (S - 1), the
    window is seq[start : min(end, n)], its last element the target, the rest the history -- the reference's
    `start = randint(0, max(0, len(seq) - 3))`, `end = randint(start + 3, start + S + 1)` (both inclusive), with the two
    uniform integers handed in.  u0, u1 are integers in [0, 2^62): for ranges up to 256 the bias of the modulo is below
    2^-54.  The draws come from torch's generator (the device's in the loader), not from Python's `random`: a run follows
    the reference's law, not its sample sequence.
    Without subsample: the last min(S, n_hist) history items, target the stored future item; u0, u1 are not read."""
    if S < 2 or n_hist < 0:
        raise ValueError(f"seq_window: S={S}, n_hist={n_hist}")
    if not subsample:
        n_items = min(S, n_hist)
        return n_hist - n_items, n_items, n_hist
    n = n_hist + 1
    start = u0 % (max(0, n - 3) + 1)
    end = min(start + 3 + u1 % (S - 1), n)
    return start, end - start - 1, end - 1


def seq_window_counts(n_hist: Tensor, draws: Optional[Tensor], S: int, subsample: bool) -> Tensor:
    """`seq_window`'s n_items for many rows at once, on the host: n_hist int64 [B] history lengths, draws int64 [B, 2]
    the rows' (u0, u1) in [0, 2^62) (not read without subsample) -> int64 [B].  The same integer operations as
    seq_window, vectorised; data/seq_loader.py uses it to know a batch's valid rows without reading the device."""
    if S < 2 or bool((n_hist < 0).any()):
        raise ValueError(f"seq_window_counts: S={S}, negative n_hist: {bool((n_hist < 0).any())}")
    n_hist = n_hist.to(torch.int64)
    if not subsample:
        return n_hist.clamp(max=S)
    n = n_hist + 1
    start = draws[:, 0] % ((n - 3).clamp(min=0) + 1)
    end = torch.minimum(start + 3 + draws[:, 1] % (S - 1), n)
    return end - start - 1


def synthetic_sequences(n_items: int, max_seq_len: int, seed: int = 4321) -> dict:
    """{split: the four CSR tensors} over n_items items: max(64, n_items // 2) users per split, history lengths spread
    over 1 .. 2 * max_seq_len (rows shorter and longer than a window both occur), uniform items."""
    out = {}
    users = max(64, n_items // 2)
    for k, split in enumerate(SEQ_SPLITS):
        g = torch.Generator().manual_seed(seed + k)
        lengths = torch.randint(1, 2 * max_seq_len + 1, (users,), generator=g)
        offsets = torch.zeros(users + 1, dtype=torch.int64)
        offsets[1:] = torch.cumsum(lengths, 0)
        out[split] = {"userId": torch.arange(users, dtype=torch.int64), "offsets": offsets,
                      "items": torch.randint(0, n_items, (int(offsets[-1]),), generator=g),
                      "itemId_fut": torch.randint(0, n_items, (users,), generator=g)}
    return out


class SeqData(Dataset):
    """User histories for the retrieval model, the reference's `SeqData` (same constructor, `max_seq_len`, `len(ds)`,
    `ds[i] -> SeqBatch`), held unpadded in CSR form per split: userId [U], offsets [U + 1], items [nnz], itemId_fut [U],
    all int64.  `is_train` selects "train", otherwise "test", as in the reference.

    Source, in order: `sequences=` (a dict {split: {the four tensors}}); `<root>/sequences.pt` holding such a dict,
    exported once from the reference's processed data ('User sequences'); a folder NAMED
    "synthetic:<N>" -- a deterministic synthetic set over N items, with a loud warning and `ds.synthetic` True.
    Anything else raises FileNotFoundError.

    `ds[i]` is the reference's row: user_ids [1], ids [max_seq_len] padded with -1, ids_fut [1], seq_mask.  (user_ids
    keeps one column, so a collated batch is the [B, 1] that modules/model.py reads.)  With `subsample` the window
    comes from `seq_window` on two draws of torch's host generator.  x and x_fut are gathered from `item_matrix`
    when one was given, with -1 rows at padded positions; without one they are -1 placeholders: the tokenizer's cached
    path, the only one the retrieval model trains on, never reads them.

    The training loop does not go through `ds[i]`: `to_device` makes the four tensors resident and
    data/seq_loader.py builds whole tokenized batches from them in one launch."""

    def __init__(self, root: str, *args, is_train: bool = True, subsample: bool = False, force_process: bool = False,
                 dataset: RecDataset = RecDataset.ML_1M, sequences: Optional[dict] = None,
                 item_matrix: Optional[Tensor] = None, **kwargs) -> None:
        del args, kwargs, force_process  # accepted for signature compatibility (split=..., etc.)
        assert (not subsample) or is_train, "Can only subsample on training split."
        self.dataset = dataset
        self.subsample = subsample
        self._max_seq_len = MAX_SEQ_LEN[dataset]
        self.split = "train" if is_train else "test"
        self.synthetic = False
        if sequences is None:
            path = os.path.join(root, "sequences.pt")
            if str(root).startswith("synthetic:"):
                n = int(str(root).split(":", 1)[1])
                print(f"[SeqData] WARNING: dataset folder {root!r} -- using SYNTHETIC user histories over {n} items; "
                      "results say nothing about a real corpus", flush=True)
                sequences = synthetic_sequences(n, self._max_seq_len)
                self.synthetic = True
            elif os.path.exists(path):
                sequences = torch.load(path, map_location="cpu", weights_only=True)
            else:
                raise FileNotFoundError(
                    f"{path} not found.  Export the user sequences first (INTEGRATION.md, 'User sequences': "
                    "torch.save({split: {'userId': [U], 'offsets': [U + 1], 'items': [nnz], 'itemId_fut': [U]} for split in "
                    "('train', 'eval', 'test')}, '<dataset_folder>/sequences.pt'), int64, eval / test rows without their "
                    "-1 padding) or opt in to synthetic histories explicitly by naming the folder 'synthetic:<n>'.")
        if self.split not in sequences:
            raise KeyError(f"SeqData: no split {self.split!r} in the sequences (found {sorted(sequences)})")
        store = sequences[self.split]
        self.userId, self.offsets, self.items, self.itemId_fut = (store[f].to(torch.int64).contiguous() for f in SEQ_FIELDS)
        U = self.userId.shape[0]
        if (self.offsets.shape != (U + 1,) or self.itemId_fut.shape != (U,) or self.items.dim() != 1 or U == 0
                or int(self.offsets[0]) != 0 or int(self.offsets[-1]) != self.items.shape[0]
                or bool((self.offsets[1:] < self.offsets[:-1]).any())):
            raise ValueError(f"SeqData: split {self.split!r} is not CSR: userId [U], offsets [U + 1] ascending from 0 to "
                             "len(items), items [nnz], itemId_fut [U]")
        self.item_data = item_matrix
        # the history lengths stay on the host when `to_device` moves the store (seq_window_counts reads them)
        self.host_lengths = (self.offsets[1:] - self.offsets[:-1]).cpu()

    @property
    def max_seq_len(self) -> int:
        return self._max_seq_len

    def to_device(self, device) -> "SeqData":
        """Make the four tensors resident on `device`; data/seq_loader.py then builds batches there.  `host_lengths`,
        the history lengths, stays a CPU tensor."""
        self.userId, self.offsets, self.items, self.itemId_fut = (
            t.to(device) for t in (self.userId, self.offsets, self.items, self.itemId_fut))
        return self

    def check_items(self, n_items: int) -> None:
        """Raise ValueError unless every stored item id lies in [0, n_items).  A one-time host check in the place of the
        reference's `ids.max()` test on every batch (modules/tokenizer/semids.py:forward)."""
        for name, t in (("items", self.items), ("itemId_fut", self.itemId_fut)):
            if t.numel() and (int(t.min()) < 0 or int(t.max()) >= n_items):
                raise ValueError(f"SeqData({self.split}): {name} holds ids in [{int(t.min())}, {int(t.max())}], outside the "
                                 f"{n_items} items of the corpus")

    def __len__(self) -> int:
        return self.userId.shape[0]

    def _features(self, ids: Tensor) -> Tensor:
        if self.item_data is None:
            return torch.full_like(ids, -1)
        x = self.item_data[ids.clamp_min(0).to(self.item_data.device), :FEATURE_DIM]
        x[(ids == -1).to(x.device)] = -1
        return x

    def __getitem__(self, idx: int) -> SeqBatch:
        idx = int(idx)
        lo, hi = int(self.offsets[idx]), int(self.offsets[idx + 1])
        S = self._max_seq_len
        u0, u1 = torch.randint(0, 2 ** 62, (2,)).tolist() if self.subsample else (0, 0)
        first, n_items, fut_pos = seq_window(hi - lo, u0, u1, S, self.subsample)
        item_ids = torch.full((S,), -1, dtype=torch.int64, device=self.items.device)
        item_ids[:n_items] = self.items[lo + first:lo + first + n_items]
        item_ids_fut = (self.itemId_fut[idx:idx + 1] if fut_pos == hi - lo else self.items[lo + fut_pos:lo + fut_pos + 1]).clone()
        assert bool((item_ids >= -1).all()), "Invalid item id found"
        return SeqBatch(user_ids=self.userId[idx:idx + 1].clone(), ids=item_ids, ids_fut=item_ids_fut,
                        x=self._features(item_ids), x_fut=self._features(item_ids_fut), seq_mask=item_ids >= 0)
