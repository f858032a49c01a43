"""T5 encoder / decoder stacks for the retrieval model (modules/model.py), in torch operators.

The reference builds its retrieval model from HuggingFace's `T5EncoderModel` and `T5Stack` with `T5Config` defaults
for everything it does not set.  This module is written for this project and reproduces what those defaults give,
with the same module tree, so a reference checkpoint loads by its state-dict names:

- d_kv = 64: each attention's inner width is heads * 64, not d_model; q/k/v/o have no bias.
- No 1/sqrt(d) scaling of the scores; a relative-position bias (32 buckets, max distance 128) lives in block 0 and is
  shared by the later blocks; bidirectional in the encoder, causal in the decoder's self-attention; none in the
  cross-attention.
- Masks are added as finfo(dtype).min; softmax in fp32.
- RMS layer norm (no mean, no bias), variance in fp32, eps 1e-6.
- ReLU feed-forward.
- Dropout 0.1 on the input embeddings, each sub-layer output, inside the feed-forward, on the attention weights and
  after the final norm.

The decoder can run incrementally: `T5Stack.forward` takes and returns a self-attention cache (one (K, V) pair per
block, [rows, heads, t, 64]) and accepts precomputed cross-attention K/V (`cross_kv`) on fewer rows than the queries:
rows r = b * beams + beam all read user b's encoder output, as the beams of a beam search do.

A stack forward chooses an attention body, a glue and a feed-forward body, then runs ONE loop over its blocks:
self-attention, cross-attention (decoder), feed-forward, with a glue call between every two bodies.  Each of the four
attributes below is "torch" (the default: the operators above) or names a fused form.  That form is taken for fp32
device tensors and a shape its kernel supports, under every setting of the other attributes; otherwise the
operators run, silently.  The module tree and the state dict are the same on every path.

- `attention_impl` = "hip": every attention call is ONE launch of ops.t5_attention (csrc/t5_attention.hip), fed the
  q / k / v Linears' outputs as they are and a [n_delta, heads] table of the relative-position bias by j - i.  Taken
  only with grad disabled, dropout inactive (eval mode) and no operator-format cache passed in.  Its incremental
  decoder keeps the self-attention K/V in per-position slabs (`T5DecodeCache`) that are written once and never copied:
  a beam search reorders an int32 ancestor table instead of the cache.
  "hip_train" is "hip" under no_grad (the same launches, decode cache included) and, with grad enabled, makes every
  attention one autograd.T5AttentionFunction call: a forward launch that keeps the row log-sum-exp instead of the
  weights, and one backward launch that recomputes them.  In train mode with dropout_rate > 0 the attention-weight
  dropout happens in the kernel; every other dropout stays torch's.  It needs one K/V per query row (beams = 1), no
  operator-format cache and a shape the backward supports.  A decode_cache under grad raises.
  `attention_long_impl` = "hip" (default "torch") goes with either: the kernel above stops at 256 queries or keys, and
  a forward with a longer attention call falls back to the operators as a whole.  With "hip" each attention call is
  chosen on its own: the kernel above where it supports the call's (Tq, Tk), else csrc/t5_attention_long.hip
  (ops.t5_attention_long, autograd.T5AttentionLongFunction; up to 2048 tokens, the keys walked in chunks with an online
  softmax, nothing of size Tq x Tk stored).  In a long-history decoder forward the self-attention stays on the short
  kernel and the cross-attention is a long call; in `generate` the cached self-attention (never more keys than levels)
  stays on the short kernel and slabs, and the cross-attention over the encoder output is ONE long launch per block and
  step, the beams of a user as the query rows of one K/V group.  With the default every answer and every launch is what
  it was without the attribute.
- `norm_impl` = "hip": the glue -- the dropout of a sub-layer's output, the residual add and the next sub-layer's RMS
  norm -- is ONE autograd.T5AddNormFunction call (csrc/t5_add_norm.hip), in eval and train mode, with and without grad:
  2 * layers + 1 calls per encoder forward, 3 * layers + 1 per decoder forward, the first on the input embeddings
  alone, the last with the final norm's weight and the dropout behind it.
- `ffn_impl` = "hip": every feed-forward body is ONE autograd.T5FFNFunction call under grad (csrc/t5_ffn.hip: one
  launch forward, at most two backward, the ReLU output the only [rows, d_ff] tensor kept) or one ops.t5_ffn_fwd
  without that tensor under no_grad, in eval and train mode; in train mode its inner dropout happens in the kernel.
- `proj_impl` = "hip": the bias-free q / k / v / o Linears around every attention are grouped calls of
  csrc/t5_proj.hip (one launch forward, at most two backward): a self-attention is ONE call for q, k and v and one for
  o, a cross-attention one for q and one for o, and `T5Stack.cross_kv` ONE call for the K/V of all blocks (eight
  weights per call: one call up to four blocks).  Under grad a call is an autograd.T5ProjFunction, whose backward adds
  the gradients of the shared input inside the kernel; under no_grad it is ops.t5_proj_fwd, and on the decode-cache
  path that call writes k and v straight into this position of the slabs.  It goes with the operator attention and
  with the fused one alike, and also needs the stack's attention weights to be fp32 device tensors that are dense and
  16-byte aligned (`hip_proj_active`).

Three more attributes say which FORM (ops.T5MatmulForm) the two matrix bodies above take.  `matmul_forms` states the
rule, once: a body that is not taken has no form, so on the "torch" bodies and on host tensors none of the three has an
effect; a stack forward (and a `cross_kv` call from outside one) resolves its forms ONCE, before its first body
(`T5Stack.matmul_plan`), and every feed-forward body and grouped projection call of that forward -- the one autograd
Function under grad, the one ops call under no_grad, `cross_kv` and the decode step's call that writes K/V into the cache
slabs included -- reads them.  They are attributes of the model or the stack, set by the caller: train_decoder.train
sets the first (amp with mixed_precision_type = "bf16") and has no parameter for the other two.

- `matmul_arith` = "fp32" (the default) or "bf16" is the arithmetic.  "bf16" rounds every operand of a matrix product to
  bf16 and accumulates in fp32 (include/rqhip.h); weights, activations, gradients and the state dict stay fp32, and so do
  the attention itself, the norms and the glue.  "fp32" ignores the other two attributes.
- `weight_images` = "none" (the default) or "bf16" (WEIGHT_IMAGES) is where the "bf16" forms get their weights.  With
  "bf16" they read bf16 IMAGES of their weights (csrc/t5_images.hip; rqhip_t5_ffn_*_bf16w / rqhip_t5_proj_*_bf16w): copies
  that hold the very roundings the bf16 kernels form in registers, in both orientations, so that forward and backward
  load a weight fragment as 16 bytes along a row and convert nothing.  Every result keeps the bits of "none".
  Each stack owns a T5WeightImages holder (`stack.images`, a plain attribute: no parameter, no buffer, nothing in the
  state dict): one bf16 arena with the images and transposed images of its blocks' wi, wo, q, k, v and o (a decoder's
  cross-attention weights included), the device job table of their one refresh launch, and a `refreshes` counter.
  Resolving the forms compares the holder's KEY -- (data_ptr, _version) of every weight and rqhip.optim.generation(),
  which every FlatAdamW.step() bumps because its kernel writes parameters without touching `_version` -- and, if it
  differs, refreshes all images with ONE launch; the same weights again cost no launch, and a refresh draws no random
  numbers.  `.to()` and `load_state_dict` drop the holder's contents.  A weight written behind the key's back (through a
  raw pointer by other code than FlatAdamW, or in place through `param.data`, which has a version counter of its own)
  needs `stack.images.invalidate()`.  Under graph capture every forward refreshes, since a replay cannot compare keys.
  Measurements: profiles/t5_weight_images.txt.
- `saved_activations` = "fp32" (the default) or "bf16" (SAVED_ACTIVATIONS) is what the "bf16" feed-forward keeps between
  its forward and its backward -- the feed-forward alone, and only under grad (rqhip_t5_ffn_*_bf16a / _bf16wa), with
  `weight_images` "none" and "bf16" alike.  With "bf16" the forward saves blocked bf16 images of dropout(relu(wi(x))) and
  of x in place of the fp32 ReLU output and the fp32 x -- 64 * ceil(rows / 32) * (d_model + d_ff) bytes per body against
  4 * rows * (d_model + d_ff) -- and no seed; the backward's active set is the image's sign, its weight-gradient kernel
  loads 16-byte bf16 fragments and neither backward kernel hashes a dropout decision.  The images hold the very operands
  the "bf16" arithmetic rounds in registers, so the loss and every gradient keep the bits of "fp32" (include/rqhip.h
  names the one difference, an activation below 2^-134).  Measured on an MI355X beside `weight_images` = "bf16" in
  alternating runs (profiles/t5_saved_activations.txt): at batch 640 a training step goes from 35.5 to 32.2 ms and, with
  the grouped projections, from 32.7 to 29.2 ms, beyond the runs' spreads, at 0.88 of the peak memory (4858 -> 4283 MiB);
  the weight-gradient kernel takes 0.28 of its twin's device time and the two row kernels 0.96 to 1.05 of theirs; at
  batch 64 no step-time difference could be measured (9.5 against 9.3 and 8.6 against 8.0 ms inside block spreads of 1.9
  to 3.7 ms).

Each of the nine attributes is validated against STACK_ATTRIBUTES at the top of every forward and `cross_kv` call, on
every path, whether or not that path consults it.

`attention_arith` = "fp32" (the default) or "bf16" is the arithmetic of the LONG attention calls alone, wherever
`attention_long_impl` = "hip" takes one: the inference launch (ops.t5_attention_long, `generate`'s cross-attention
included), and under grad the forward and backward of autograd.T5AttentionLongFunction.  "bf16" rounds q, k, v,
d_out, the unnormalised weights and dS to bf16 as matrix operands and keeps the softmax, its sums and every stored
tensor fp32 (include/rqhip.h, rqhip_t5_attention_long_*_bf16).  The short kernel (up to 256 tokens), and with it the
cached decode step, stays fp32; `matmul_arith` does not touch the attention and this attribute does not touch the matrix
forms.  With `attention_long_impl` = "torch" or host tensors it has no effect.  It is an attribute of the model or the
stack, set by the caller: train_decoder.train has no parameter for it.  Measured on an MI355X at batch 64 and 1025
encoder tokens in one alternating run (profiles/t5_attention_long_bf16.txt): one encoder forward + backward 46.8 ms
against the fp32 arm's 75.3 ms and the operators' 72.1 ms, one `generate` 12.4 against 15.5 and 31.9 ms, at the fp32
arm's peak memory; the four bf16 kernels take 0.53 of their fp32 twins' device time.

Packed rows.  An encoder forward can run on the valid tokens of variable-length rows alone: `T5Stack.forward(inputs_embeds
[1, N, d], packed=PackedRows(cu, bound, batch, N))` takes the batch's rows one behind the other, row b at tokens cu[b] ..
cu[b + 1] - 1 (cu: int32 [batch + 1] on the device, every row at most `bound` tokens, N known to the host), and returns
[1, N, d]; the decoder reads such an output with `encoder_hidden_states` [1, N, d] and `encoder_packed=` the same record
(`cross_kv` takes the [1, N, d] tensor as it is).  It is selected by these ARGUMENTS, not by a stack attribute, and
takes no mask: every packed token is valid.  Only the attention needs the rows' structure: each self-attention of the
encoder and each cross-attention of the decoder is ONE packed call (ops.t5_attention_packed under no_grad,
autograd.T5AttentionPackedFunction under grad; csrc/t5_attention.hip), which keeps the padded call's bias index, dropout
element index, kernel instantiation and LDS layout and shortens each workgroup's loops to its row's own length, so that
on every valid token it has the bits of the padded call with the prefix key mask.  The glue, the feed-forward and the
grouped projections run unchanged on the N rows: their kernels take any row count and a row's result does not depend
on the batch (include/rqhip.h), so in eval mode the loss keeps the padded path's bits (weight gradients sum the rows in
other groups and differ by rounding).  In train mode a row-local dropout decision is a function of the element's index
among the N rows, so a packed step draws other masks than a padded one: the same law, another sample.  Packed rows need
the fused attention this forward is in anyway (`T5Stack._attention_mode`, which `packed_rows_active` asks as the other two
attention predicates do) and every length within the short kernel's 256; elsewhere they raise -- modules/model.py checks
before it packs and runs the padded path instead.  N depends on the data, so a packed forward cannot be replayed from a
captured graph.
A decoder forward with `encoder_packed` may also be the cached decode step of a beam search, under no_grad: it takes
`cross_kv` (of the [1, N, d] encoder output) and a `decode_cache` beside `encoder_packed`, with R = batch * beams query
rows, rows b * beams .. of which read encoder row b.  Its self-attention stays on the slabs and the short kernel, as
without packed rows; its cross-attention is ONE ops.t5_attention_packed_beams call per block (csrc/t5_attention.hip, the
same kernel body: the dense arm's groups of beams over the packed arm's K/V), which on every query has the bits of the
padded call with the prefix key mask, and at beams = 1 (the first step) those of ops.t5_attention_packed.  The same call
serves a forward without a cache whose query rows outnumber the encoder rows; with as many query rows as encoder rows
and no cache the cross-attention is the packed call above.  `packed_rows_active` is asked with the step's query length
1.  What still raises with packed rows: an `encoder_attention_mask` or `attention_mask`, an operator-format
`past_key_values`, and grad enabled with beams > 1 or with a decode_cache (there is no backward for the beams).

The fused forms take their dropout seeds as int64s drawn on the device with torch.randint (the default generator:
torch.manual_seed reproduces a run), none in eval mode or at dropout_rate 0.  The fused attention draws one per call.
With the "hip" glue a stack forward draws once before its first body, one seed per glue call and behind them one per
fused feed-forward; with the operator glue each fused feed-forward draws its own, immediately before its sub-layer.
"""
import math
from typing import List, NamedTuple, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from rqhip import ops, optim
from rqhip.autograd import (T5AddNormFunction, T5AttentionFunction, T5AttentionLongFunction, T5AttentionPackedFunction,
                            T5FFNFunction, T5ProjFunction)

KV = Tuple[Tensor, Tensor]
ATTENTION_IMPLS = ("torch", "hip", "hip_train")
ATTENTION_LONG_IMPLS = ("torch", "hip")
NORM_IMPLS = ("torch", "hip")
FFN_IMPLS = ("torch", "hip")
PROJ_IMPLS = ("torch", "hip")
MATMUL_ARITHS = ops.T5_ARITHS  # ("fp32", "bf16")
ATTENTION_ARITHS = ops.T5_ARITHS  # of the long attention calls
WEIGHT_IMAGES = ("none", "bf16")  # where the "bf16" matrix forms read their weights: as stored, or from bf16 images
SAVED_ACTIVATIONS = ops.T5_SAVED  # ("fp32", "bf16"): what the "bf16" feed-forward saves for its backward
# the attributes of a T5Stack that choose its bodies (the model hands its own to both stacks), and what each may be
STACK_ATTRIBUTES = {"attention_impl": ATTENTION_IMPLS, "attention_long_impl": ATTENTION_LONG_IMPLS,
                    "norm_impl": NORM_IMPLS, "ffn_impl": FFN_IMPLS, "proj_impl": PROJ_IMPLS,
                    "matmul_arith": MATMUL_ARITHS, "attention_arith": ATTENTION_ARITHS, "weight_images": WEIGHT_IMAGES,
                    "saved_activations": SAVED_ACTIVATIONS}
MAX_DELTA_BUCKETS = 64  # delta ranges a T5Attention keeps the integer buckets of


def checked(owner, name: str):
    """The attribute `name` (of STACK_ATTRIBUTES) of a stack or a model, validated."""
    value, allowed = getattr(owner, name), STACK_ATTRIBUTES[name]
    if value not in allowed:
        raise ValueError(f"{name} must be one of {allowed}, got {value!r}")
    return value


def matmul_forms(arith: str, weight_images: str, saved_activations: str, ffn_active: bool, proj_active: bool,
                 grad_enabled: bool):
    """The forms (ops.T5MatmulForm) of a forward's "hip" feed-forward bodies and grouped projections, from the three
    attributes (valid values) and which of the two bodies are taken -> (ffn form, proj form).  A body that is not taken
    has None.  "fp32" ignores the other two attributes; with "bf16" both bodies read weight images where `weight_images`
    is "bf16", and the feed-forward -- it alone, and only under grad, where there is a backward to save for -- keeps
    bf16 saved activations where `saved_activations` is "bf16"."""
    bf16 = arith == "bf16"
    images = bf16 and weight_images == "bf16"
    saved = bf16 and saved_activations == "bf16" and grad_enabled
    return (ops.T5MatmulForm(arith, images, saved) if ffn_active else None,
            ops.T5MatmulForm(arith, images, False) if proj_active else None)


class PackedRows(NamedTuple):
    """Variable-length rows without their padding (module docstring, "Packed rows"): `batch` rows of at most `bound`
    tokens lie one behind the other in a [1, N, d] tensor, row b at tokens cu[b] .. cu[b + 1] - 1.  `cu` is an int32
    [batch + 1] DEVICE tensor; `rows` = N = cu[batch] is the tensor's own size, known to the host without reading it."""
    cu: Tensor
    bound: int
    batch: int
    rows: int   # N


class T5Config:
    def __init__(self, vocab_size: int, d_model: int = 512, num_heads: int = 8, d_ff: int = 2048, num_layers: int = 6,
                 d_kv: int = 64, relative_attention_num_buckets: int = 32, relative_attention_max_distance: int = 128,
                 dropout_rate: float = 0.1, layer_norm_epsilon: float = 1e-6, is_decoder: bool = False) -> None:
        self.vocab_size = vocab_size
        self.d_model = d_model
        self.num_heads = num_heads
        self.d_ff = d_ff
        self.num_layers = num_layers
        self.d_kv = d_kv
        self.relative_attention_num_buckets = relative_attention_num_buckets
        self.relative_attention_max_distance = relative_attention_max_distance
        self.dropout_rate = dropout_rate
        self.layer_norm_epsilon = layer_norm_epsilon
        self.is_decoder = is_decoder


def additive_mask(mask: Tensor, dtype: torch.dtype) -> Tensor:
    """[B, S] keep-mask (1 = attend) -> [B, 1, 1, S] additive mask: 0 where kept, finfo.min where masked."""
    return (1.0 - mask[:, None, None, :].to(dtype)) * torch.finfo(dtype).min


class T5LayerNorm(nn.Module):
    def __init__(self, d_model: int, eps: float = 1e-6) -> None:
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d_model))
        self.variance_epsilon = eps

    def forward(self, x: Tensor) -> Tensor:
        variance = x.to(torch.float32).pow(2).mean(-1, keepdim=True)
        x = x * torch.rsqrt(variance + self.variance_epsilon)
        return self.weight * x


def relative_position_bucket(relative_position: Tensor, bidirectional: bool, num_buckets: int,
                             max_distance: int) -> Tensor:
    """T5's bucketing of memory_position - query_position: exact buckets for small distances, logarithmic bins up to
    max_distance; bidirectional halves the buckets between the two signs, causal clamps positive offsets to 0."""
    buckets = torch.zeros_like(relative_position)
    if bidirectional:
        num_buckets //= 2
        buckets = buckets + (relative_position > 0).to(torch.long) * num_buckets
        relative_position = relative_position.abs()
    else:
        relative_position = -torch.min(relative_position, torch.zeros_like(relative_position))
    max_exact = num_buckets // 2
    is_small = relative_position < max_exact
    large = max_exact + (torch.log(relative_position.float() / max_exact) / math.log(max_distance / max_exact)
                         * (num_buckets - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, num_buckets - 1))
    return buckets + torch.where(is_small, relative_position, large)


class T5DecodeCache:
    """Self-attention K/V of an incremental decode on the "hip" path.  Block i owns two slabs [steps, rows, heads * 64]:
    position t's projections of every row alive at step t, written once.  `anc` [rows, steps] int32 says where a row's
    history lives: its key at position t < pos is row anc[r, t] of slab t (its own key at `pos` is row r of slab
    `pos`).  `reorder(parent)` moves to the next position after a beam step: new row r continues old row parent[r]."""

    def __init__(self, num_blocks: int, steps: int, rows: int, inner: int, device) -> None:
        self.slabs = [(torch.empty(steps, rows, inner, device=device), torch.empty(steps, rows, inner, device=device))
                      for _ in range(num_blocks)]
        self.anc = torch.zeros(rows, steps, dtype=torch.int32, device=device)
        self.steps, self.rows, self.pos = steps, rows, 0

    def reorder(self, parent: Tensor) -> None:
        self.anc = advance_ancestors(self.anc, parent, self.pos)
        self.pos += 1


def advance_ancestors(anc: Tensor, parent: Tensor, pos: int) -> Tensor:
    """The ancestor table after position `pos`: row r of the result continues old row parent[r] -- its columns < pos
    are that row's (one small gather), column `pos` is parent[r] itself."""
    parent = parent.reshape(-1)
    out = anc.index_select(0, parent)
    out[:, pos] = parent
    return out


def _draw_seed(p: float, device, n: int = 1) -> Optional[Tensor]:
    """Dropout seeds of fused calls: n int64s from one draw on the device, never read by the host."""
    return torch.randint(0, 2 ** 62, (n,), dtype=torch.int64, device=device) if p > 0 else None


class _Seeds:
    """Where the seeds of a stack forward's glue and feed-forward calls come from (module docstring).  n_glue > 0 (the
    "hip" glue): one draw now of n_glue + n_ffn seeds, a call gets a one-element view; else every feed-forward draws."""

    def __init__(self, p: float, device, n_glue: int, n_ffn: int) -> None:
        self.p, self.device, self.n_glue = p, device, n_glue
        self.drawn = _draw_seed(p, device, n_glue + n_ffn) if n_glue else None

    def glue(self, k: int) -> Optional[Tensor]:
        return None if self.drawn is None else self.drawn[k:k + 1]

    def ffn(self, i: int) -> Optional[Tensor]:
        return self.glue(self.n_glue + i) if self.n_glue else _draw_seed(self.p, self.device)


class T5WeightImages:
    """The bf16 weight images of one T5Stack (module docstring, `weight_images`): one arena, an (image, transposed
    image) pair per weight, the device job table of the refresh launch, the key the images were made under, and
    `refreshes`, the number of refresh launches so far."""

    def __init__(self) -> None:
        self.refreshes = 0
        self.invalidate()

    def invalidate(self) -> None:
        """Forget the images: the next use allocates and refreshes."""
        self.key = None       # ((data_ptr, _version) of every weight ..., optim.generation()) of the last refresh
        self.arena = None
        self.jobs = None
        self.pairs = {}       # id(weight) -> (image, transposed image)

    @staticmethod
    def key_of(weights) -> tuple:
        """What decides whether images of `weights` are current: where each weight lives, how often torch has seen it
        written (in-place operators, copy_ of load_state_dict, torch.optim steps), and how many FlatAdamW steps, whose
        kernel writes through raw pointers, this process has made."""
        return tuple((w.data_ptr(), w._version) for w in weights) + (optim.generation(),)

    def current(self, weights) -> bool:
        return self.key is not None and self.key == self.key_of(weights)

    def ensure(self, weights) -> "T5WeightImages":
        """Make the images those of `weights` (a list of fp32 device Parameters): nothing when the key stands, else ONE
        launch; the arena and the job table are rebuilt only when a weight has moved."""
        key = self.key_of(weights)
        capturing = torch.cuda.is_current_stream_capturing()
        if key == self.key and not capturing:
            return self
        if self.key is None or [k[0] for k in key[:-1]] != [k[0] for k in self.key[:-1]]:
            datas = [w.detach() for w in weights]
            self.arena, imgs, imgs_t = ops.bf16_images_alloc(datas)
            self.jobs = ops.bf16_images_jobs(datas, imgs, imgs_t)
        ops.bf16_images(self.jobs)
        self.refreshes += 1
        self.pairs = {id(w): pair for w, pair in zip(weights, zip(self.jobs.tensors[1], self.jobs.tensors[2]))}
        self.key = key
        return self

    def of(self, weight: Tensor):
        """(image, transposed image) of one of the weights of the last `ensure`."""
        return self.pairs[id(weight)]


class MatmulPlan(NamedTuple):
    """What one stack forward resolved about its matrix bodies (T5Stack.matmul_plan): `matmul_forms`' pair and, where
    either form reads weight images, the stack's holder with current images."""
    ffn: Optional[ops.T5MatmulForm] = None
    proj: Optional[ops.T5MatmulForm] = None
    images: Optional[T5WeightImages] = None


def _project(plan: MatmulPlan, x: Tensor, linears, outs=None) -> Tuple[Tensor, ...]:
    """The bias-free Linears `linears` of the same x -> their outputs: the operators one by one where the plan has no
    proj form, else ONE call for the group in that form (T5ProjFunction under grad, ops.t5_proj_fwd under no_grad, which
    writes into `outs` where given)."""
    form = plan.proj
    if form is None:
        return tuple(lin(x) for lin in linears)
    weights = [lin.weight for lin in linears]
    imgs, imgs_t = zip(*[plan.images.of(w) for w in weights]) if form.images else ((), ())
    if torch.is_grad_enabled():
        return T5ProjFunction.apply(x, form, *weights, *imgs, *imgs_t)
    return ops.t5_proj_fwd(x, weights, outs, **form.keywords(imgs))


def _attend(module: nn.Module, q: Tensor, k: Tensor, v: Tensor, bias: Optional[Tensor], mask: Optional[Tensor]) -> Tensor:
    scores = torch.matmul(q, k.transpose(-1, -2))
    if bias is not None:
        scores = scores + bias
    if mask is not None:
        scores = scores + mask
    weights = F.softmax(scores.float(), dim=-1).type_as(scores)
    weights = F.dropout(weights, p=module.dropout, training=module.training)
    return torch.matmul(weights, v)


class T5Attention(nn.Module):
    def __init__(self, config: T5Config, has_relative_attention_bias: bool = False) -> None:
        super().__init__()
        self.is_decoder = config.is_decoder
        self.has_relative_attention_bias = has_relative_attention_bias
        self.num_buckets = config.relative_attention_num_buckets
        self.max_distance = config.relative_attention_max_distance
        self.n_heads = config.num_heads
        self.d_kv = config.d_kv
        self.dropout = config.dropout_rate
        inner = self.n_heads * self.d_kv
        self.q = nn.Linear(config.d_model, inner, bias=False)
        self.k = nn.Linear(config.d_model, inner, bias=False)
        self.v = nn.Linear(config.d_model, inner, bias=False)
        self.o = nn.Linear(inner, config.d_model, bias=False)
        if has_relative_attention_bias:
            self.relative_attention_bias = nn.Embedding(self.num_buckets, self.n_heads)
        self._delta_buckets = {}  # (lowest delta, highest + 1, device) -> integer buckets of that range of j - i - past

    def compute_bias(self, query_length: int, key_length: int, past: int = 0) -> Tensor:
        """[1, heads, query_length, key_length] bias for queries at positions past .. past + query_length - 1."""
        dev = self.relative_attention_bias.weight.device
        context = torch.arange(query_length, dtype=torch.long, device=dev)[:, None] + past
        memory = torch.arange(key_length, dtype=torch.long, device=dev)[None, :]
        bucket = relative_position_bucket(memory - context, bidirectional=not self.is_decoder,
                                          num_buckets=self.num_buckets, max_distance=self.max_distance)
        return self.relative_attention_bias(bucket).permute(2, 0, 1).unsqueeze(0)

    def delta_table(self, query_length: int, key_length: int, past: int = 0) -> Tuple[Tensor, int]:
        """(table [n_delta, heads], offset) with table[(j - i - past) + offset, h] == compute_bias(...)[0, h, i, j]: the
        bias depends on j - i - past alone.  The integer buckets (relative_position_bucket, on the weight's device as
        in compute_bias) are kept per shape; the table is one gather of the embedding weight."""
        dev = self.relative_attention_bias.weight.device
        lo, hi = -(query_length - 1) - past, key_length - past  # the deltas lo .. hi - 1 decide the buckets
        key = (lo, hi, dev)
        bucket = self._delta_buckets.get(key)
        if bucket is None:
            delta = torch.arange(lo, hi, dtype=torch.long, device=dev)
            bucket = relative_position_bucket(delta, bidirectional=not self.is_decoder, num_buckets=self.num_buckets,
                                              max_distance=self.max_distance)
            if not (dev.type == "cuda" and torch.cuda.is_current_stream_capturing()):
                if len(self._delta_buckets) >= MAX_DELTA_BUCKETS:  # variable lengths: start over, never grow
                    self._delta_buckets.clear()
                self._delta_buckets[key] = bucket  # memory of a graph's pool must not outlive the capture
        return self.relative_attention_bias(bucket), query_length - 1 + past

    def _heads(self, x: Tensor) -> Tensor:  # [R, T, inner] -> [R, heads, T, d_kv]
        return x.view(x.shape[0], x.shape[1], self.n_heads, self.d_kv).transpose(1, 2)

    def project_kv(self, x: Tensor) -> KV:
        return self._heads(self.k(x)), self._heads(self.v(x))

    def self_attention(self, x: Tensor, bias: Optional[Tensor], mask: Optional[Tensor], past: Optional[KV],
                       plan: MatmulPlan = MatmulPlan()) -> Tuple[Tensor, KV]:
        """plan: with a proj form the projections are grouped calls (`_project`): one for q, k and v, one for o."""
        q, k, v = (self._heads(t) for t in _project(plan, x, (self.q, self.k, self.v)))
        if past is not None:
            k, v = torch.cat([past[0], k], dim=2), torch.cat([past[1], v], dim=2)
        out = _attend(self, q, k, v, bias, mask)
        return _project(plan, out.transpose(1, 2).reshape(x.shape[0], x.shape[1], -1), (self.o,))[0], (k, v)

    def cross_attention(self, x: Tensor, kv: KV, mask: Optional[Tensor], plan: MatmulPlan = MatmulPlan()) -> Tensor:
        """Queries x [R, T, d] with R = B * beams over keys / values [B, heads, S, d_kv] of B rows."""
        R, T = x.shape[0], x.shape[1]
        B = kv[0].shape[0]
        beams = R // B
        q = self._heads(_project(plan, x, (self.q,))[0])  # [R, H, T, dk]
        if beams != 1:
            q = q.view(B, beams, self.n_heads, T, self.d_kv).transpose(1, 2).reshape(B, self.n_heads, beams * T,
                                                                                      self.d_kv)
        out = _attend(self, q, kv[0], kv[1], None, mask)
        if beams != 1:
            out = out.view(B, self.n_heads, beams, T, self.d_kv).transpose(1, 2).reshape(R, self.n_heads, T, self.d_kv)
        return _project(plan, out.transpose(1, 2).reshape(R, T, -1), (self.o,))[0]


class _OperatorAttention:
    """The attention bodies of a stack forward as torch operators: the bias and the additive masks are built once."""

    def __init__(self, stack: "T5Stack", inputs_embeds: Tensor, attention_mask: Optional[Tensor],
                 encoder_hidden_states: Optional[Tensor], encoder_attention_mask: Optional[Tensor],
                 past_key_values: Optional[List[KV]], cross_kv: Optional[List[KV]], plan: MatmulPlan) -> None:
        T, dtype = inputs_embeds.shape[1], inputs_embeds.dtype
        past = 0 if past_key_values is None else past_key_values[0][0].shape[2]
        keys = past + T
        keep = None if attention_mask is None else attention_mask[:, None, None, :].bool()
        if stack.is_decoder and T > 1:
            causal = torch.ones(T, keys, dtype=torch.bool, device=inputs_embeds.device).tril(diagonal=past)[None, None]
            keep = causal if keep is None else keep & causal
        self.mask = None if keep is None else (~keep).to(dtype) * torch.finfo(dtype).min
        self.bias = stack.block[0].layer[0].SelfAttention.compute_bias(T, keys, past)
        self.past_key_values = past_key_values
        self.plan = plan
        if stack.is_decoder:
            self.cross_kv = stack.cross_kv(encoder_hidden_states, plan) if cross_kv is None else cross_kv
            self.cross_mask = None if encoder_attention_mask is None else additive_mask(encoder_attention_mask, dtype)

    def self_attention(self, i: int, module: T5Attention, normed: Tensor) -> Tuple[Tensor, KV]:
        return module.self_attention(normed, self.bias, self.mask,
                                     None if self.past_key_values is None else self.past_key_values[i], self.plan)

    def cross_attention(self, i: int, module: T5Attention, normed: Tensor) -> Tensor:
        return module.cross_attention(normed, self.cross_kv[i], self.cross_mask, self.plan)


class _HipAttention:
    """The attention bodies of a stack forward on the "hip" path: the bias table and the byte masks are built once,
    every attention is one launch (`train`: one T5AttentionFunction call, with the attention-weight dropout of train
    mode in the kernel, from a seed drawn per call).  `plan`: with a proj form the projections around it are grouped
    calls (`_project`).  The long calls run in the stack's attention_arith."""

    def __init__(self, stack: "T5Stack", T: int, attention_mask: Optional[Tensor],
                 encoder_attention_mask: Optional[Tensor], cross_kv: Optional[List[KV]],
                 cache: Optional[T5DecodeCache], train: bool, plan: MatmulPlan, packed: Optional[PackedRows] = None,
                 encoder_packed: Optional[PackedRows] = None) -> None:
        """packed: the stack's own rows are packed ([1, N, d], T = packed.bound): every self-attention is a packed
        call with both tables.  encoder_packed: the encoder output is ([1, N, d]): every cross-attention is a packed
        call of the dense queries over packed K/V -- on the cached decode step (`cache`, no_grad), and wherever the
        query rows outnumber the encoder rows, ONE ops.t5_attention_packed_beams call, the beams of a user as the query
        rows of its packed row.  Neither takes a mask: every packed token is valid."""
        self.packed, self.encoder_packed = packed, encoder_packed
        self.train, self.plan = train, plan
        self.long = stack.attention_long_impl == "hip"  # calls the short kernel does not support go to the long one
        self.long_for = {}  # (Tq, Tk) -> whether that call is a long one
        self.long_arith = stack.attention_arith
        self.long_kw = {} if self.long_arith == "fp32" else {"arith": self.long_arith}  # the keyword only off the default
        self.p = float(stack.config.dropout_rate) if train and stack.training else 0.0
        self.cache = cache
        self.past = 0 if cache is None else cache.pos
        self.table, self.offset = stack.block[0].layer[0].SelfAttention.delta_table(T, self.past + T, self.past)
        self.key_mask = None if attention_mask is None else attention_mask.bool()
        self.causal = stack.is_decoder and T > 1
        self.cross_kv = cross_kv
        self.cross_mask = None if encoder_attention_mask is None else encoder_attention_mask.bool()

    def _launch(self, module: T5Attention, q: Tensor, k: Tensor, v: Tensor, table: Optional[Tensor], offset: int,
                key_mask: Optional[Tensor], causal: bool) -> Tensor:
        shape = (q.shape[1], k.shape[1])
        if self.long and shape not in self.long_for:  # asked once per shape: the self-attention's, the cross-attention's
            self.long_for[shape] = not ops.t5_attention_supported(q.dtype, module.d_kv, module.n_heads, *shape)
        long = self.long and self.long_for[shape]
        if self.train:
            call = (q, k, v, table, module.n_heads, offset, key_mask, causal, self.p, _draw_seed(self.p, q.device))
            return T5AttentionLongFunction.apply(*call, self.long_arith) if long else T5AttentionFunction.apply(*call)
        if long:
            return ops.t5_attention_long(q, k, v, module.n_heads, bias_by_delta=table, bias_offset=offset,
                                         key_mask=key_mask, causal=causal, **self.long_kw)
        return ops.t5_attention(q, k, v, module.n_heads, bias_by_delta=table, bias_offset=offset, key_mask=key_mask,
                                causal=causal)

    def _launch_packed(self, module: T5Attention, q: Tensor, k: Tensor, v: Tensor, table: Optional[Tensor], offset: int,
                       q_rows: Optional[PackedRows], k_rows: PackedRows) -> Tensor:
        """One packed call (ops.t5_attention_packed, under grad autograd.T5AttentionPackedFunction): k, v [N, inner]
        by k_rows; q [N, inner] by q_rows, or dense [R, Tq, inner] without."""
        cu_q, max_q = (None, None) if q_rows is None else (q_rows.cu, q_rows.bound)
        if self.train:
            return T5AttentionPackedFunction.apply(q, k, v, table, module.n_heads, offset, cu_q, k_rows.cu, max_q,
                                                   k_rows.bound, self.p, _draw_seed(self.p, q.device))
        return ops.t5_attention_packed(q, k, v, module.n_heads, cu_q=cu_q, cu_k=k_rows.cu, max_q=max_q,
                                       max_k=k_rows.bound, bias_by_delta=table, bias_offset=offset)

    def self_attention(self, i: int, module: T5Attention, normed: Tensor) -> Tuple[Tensor, KV]:
        """One launch; with a decode cache the K/V projections go straight into block i's slabs."""
        if self.packed is not None:
            q, k, v = _project(self.plan, normed, (module.q, module.k, module.v))       # [1, N, inner]
            # (squeeze, not [0]: a view in the backward too, where a select would zero-fill and copy its gradient)
            out = self._launch_packed(module, q.squeeze(0), k.squeeze(0), v.squeeze(0), self.table, self.offset,
                                      self.packed, self.packed)
            return _project(self.plan, out.unsqueeze(0), (module.o,))[0], (module._heads(k), module._heads(v))
        if self.cache is None:
            q, k, v = _project(self.plan, normed, (module.q, module.k, module.v))
            out = self._launch(module, q, k, v, self.table, self.offset, self.key_mask, self.causal)
            return _project(self.plan, out, (module.o,))[0], (module._heads(k), module._heads(v))
        R = normed.shape[0]
        ks, vs = self.cache.slabs[i]
        if self.plan.proj:  # q into a new tensor, k and v into this position of the slabs: one launch
            q = _project(self.plan, normed, (module.q, module.k, module.v),
                         [None, ks[self.past, :R], vs[self.past, :R]])[0]
        else:
            q = module.q(normed)
            x2 = normed.reshape(R, -1)
            torch.mm(x2, module.k.weight.t(), out=ks[self.past, :R])
            torch.mm(x2, module.v.weight.t(), out=vs[self.past, :R])
        out = ops.t5_attention(q, ks, vs, module.n_heads, bias_by_delta=self.table, bias_offset=self.offset,
                               past=self.past, anc=self.cache.anc[:R])
        return _project(self.plan, out, (module.o,))[0], (ks, vs)

    def cross_attention(self, i: int, module: T5Attention, normed: Tensor) -> Tensor:
        """One launch: the beams of a user are the query rows of one K/V group."""
        # a view of the Linear's output
        k, v = (t.transpose(1, 2).reshape(t.shape[0], t.shape[2], -1) for t in self.cross_kv[i])
        q = _project(self.plan, normed, (module.q,))[0]
        if self.encoder_packed is not None:
            rows = self.encoder_packed
            beams = q.shape[0] // rows.batch
            if self.cache is not None or beams > 1:  # the decode step (no_grad): the beams of a user over its packed row
                out = ops.t5_attention_packed_beams(q, k.squeeze(0), v.squeeze(0), module.n_heads, cu_k=rows.cu,
                                                    max_k=rows.bound, beams=beams)
            else:
                out = self._launch_packed(module, q, k.squeeze(0), v.squeeze(0), None, 0, None, rows)
            return _project(self.plan, out, (module.o,))[0]
        return _project(self.plan, self._launch(module, q, k, v, None, 0, self.cross_mask, False), (module.o,))[0]


class T5LayerSelfAttention(nn.Module):
    """A sub-layer's body, norm and dropout, as T5LayerCrossAttention and T5LayerFF are; T5Stack.forward drives them."""

    def __init__(self, config: T5Config, has_relative_attention_bias: bool = False) -> None:
        super().__init__()
        self.SelfAttention = T5Attention(config, has_relative_attention_bias)
        self.layer_norm = T5LayerNorm(config.d_model, eps=config.layer_norm_epsilon)
        self.dropout = nn.Dropout(config.dropout_rate)


class T5LayerCrossAttention(nn.Module):
    def __init__(self, config: T5Config) -> None:
        super().__init__()
        self.EncDecAttention = T5Attention(config, has_relative_attention_bias=False)
        self.layer_norm = T5LayerNorm(config.d_model, eps=config.layer_norm_epsilon)
        self.dropout = nn.Dropout(config.dropout_rate)


class T5DenseReluDense(nn.Module):
    def __init__(self, config: T5Config) -> None:
        super().__init__()
        self.wi = nn.Linear(config.d_model, config.d_ff, bias=False)
        self.wo = nn.Linear(config.d_ff, config.d_model, bias=False)
        self.dropout = nn.Dropout(config.dropout_rate)

    def forward(self, x: Tensor) -> Tensor:
        return self.wo(self.dropout(F.relu(self.wi(x))))

    def forward_hip(self, x: Tensor, p: float, seed: Optional[Tensor], plan: MatmulPlan) -> Tensor:
        """forward as one fused call (the "hip" feed-forward body) in the plan's ffn form, its dropout at rate p from
        `seed`: T5FFNFunction under grad, ops.t5_ffn_fwd without the tensors a backward would need under no_grad."""
        form, wi, wo = plan.ffn, self.wi.weight, self.wo.weight
        (wi16, wi16t), (wo16, wo16t) = (plan.images.of(wi), plan.images.of(wo)) if form.images else ((None, None),) * 2
        if torch.is_grad_enabled():
            return T5FFNFunction.apply(x, wi, wo, p, seed, form, wi16, wo16, wi16t, wo16t)
        return ops.t5_ffn_fwd(x, wi, wo, p, seed, need_h=False, **form.keywords((wi16, wo16)))[0]


class T5LayerFF(nn.Module):
    def __init__(self, config: T5Config) -> None:
        super().__init__()
        self.DenseReluDense = T5DenseReluDense(config)
        self.layer_norm = T5LayerNorm(config.d_model, eps=config.layer_norm_epsilon)
        self.dropout = nn.Dropout(config.dropout_rate)


class T5Block(nn.Module):
    def __init__(self, config: T5Config, has_relative_attention_bias: bool = False) -> None:
        super().__init__()
        layers = [T5LayerSelfAttention(config, has_relative_attention_bias)]
        if config.is_decoder:
            layers.append(T5LayerCrossAttention(config))
        layers.append(T5LayerFF(config))
        self.layer = nn.ModuleList(layers)


class T5Stack(nn.Module):
    def __init__(self, config: T5Config, embed_tokens: Optional[nn.Embedding] = None) -> None:
        super().__init__()
        self.config = config
        self.is_decoder = config.is_decoder
        # the stacks are driven with inputs_embeds; the table is kept for the state-dict layout
        self.embed_tokens = embed_tokens if embed_tokens is not None else nn.Embedding(config.vocab_size,
                                                                                       config.d_model)
        self.block = nn.ModuleList([T5Block(config, has_relative_attention_bias=(i == 0))
                                    for i in range(config.num_layers)])
        self.final_layer_norm = T5LayerNorm(config.d_model, eps=config.layer_norm_epsilon)
        self.dropout = nn.Dropout(config.dropout_rate)
        self.attention_impl = "torch"  # or "hip" / "hip_train": see the module docstring
        self.attention_long_impl = "torch"  # or "hip": the fused attention beyond 256 tokens (module docstring)
        self.norm_impl = "torch"  # or "hip": see the module docstring
        self.ffn_impl = "torch"  # or "hip": see the module docstring
        self.proj_impl = "torch"  # or "hip": see the module docstring
        self.matmul_arith = "fp32"  # or "bf16": the arithmetic of the "hip" feed-forward and projections (docstring)
        self.attention_arith = "fp32"  # or "bf16": the arithmetic of the long attention calls (module docstring)
        self.weight_images = "none"  # or "bf16": the "bf16" matrix forms read bf16 images of their weights (docstring)
        self.saved_activations = "fp32"  # or "bf16": what the "bf16" feed-forward saves for its backward (docstring)
        self.images = T5WeightImages()  # plain attribute: not a parameter, not a buffer, not in the state dict
        init_t5_weights(self, config)

    def _apply(self, fn, *args, **kwargs):
        self.images.invalidate()  # .to() / .cuda() / .float(): the weights move
        return super()._apply(fn, *args, **kwargs)

    def _load_from_state_dict(self, *args, **kwargs):
        self.images.invalidate()  # load_state_dict: the weights change (their _version says so too)
        return super()._load_from_state_dict(*args, **kwargs)

    def image_weights(self, ffn: bool, proj: bool) -> List[Tensor]:
        """The weights the holder keeps images of, in block order: the feed-forward's with `ffn`, the attentions'
        (cross-attention included) with `proj`."""
        weights = []
        for blk in self.block:
            if proj:
                weights += [lin.weight for layer in list(blk.layer)[:-1] for att in layer.children()
                            if isinstance(att, T5Attention) for lin in (att.q, att.k, att.v, att.o)]
            if ffn:
                dense = blk.layer[-1].DenseReluDense
                weights += [dense.wi.weight, dense.wo.weight]
        return weights

    def validate(self) -> None:
        """Every attribute of STACK_ATTRIBUTES is one of its values, or ValueError."""
        for name in STACK_ATTRIBUTES:
            checked(self, name)

    # one attribute each, validated
    def arith(self) -> str:
        return checked(self, "matmul_arith")

    def attention_arithmetic(self) -> str:
        return checked(self, "attention_arith")

    def weight_images_mode(self) -> str:
        return checked(self, "weight_images")

    def saved_activations_mode(self) -> str:
        return checked(self, "saved_activations")

    def matmul_plan(self, x: Tensor) -> MatmulPlan:
        """What a forward of x does about its matrix bodies, resolved once: `matmul_forms` of the (valid) attributes and
        of which "hip" bodies x takes, and where a form reads weight images the holder, refreshed here by one launch if
        its key differs."""
        ffn, proj = matmul_forms(self.matmul_arith, self.weight_images, self.saved_activations, self.hip_ffn_active(x),
                                 self.hip_proj_active(x), torch.is_grad_enabled())
        reads_images = any(form is not None and form.images for form in (ffn, proj))
        images = self.images.ensure(self.image_weights(ffn is not None, proj is not None)) if reads_images else None
        return MatmulPlan(ffn, proj, images)

    def cross_kv(self, encoder_hidden_states: Tensor, plan: Optional[MatmulPlan] = None) -> List[KV]:
        """Cross-attention K/V of every block, computed once per encoder output (proj_impl = "hip": by one grouped
        call for all blocks, one per four blocks beyond that).  plan: the forward's; a call from outside a forward
        validates the attributes and resolves its own."""
        if plan is None:
            self.validate()
            plan = self.matmul_plan(encoder_hidden_states)
        atts = [blk.layer[1].EncDecAttention for blk in self.block]
        if plan.proj is None:
            return [att.project_kv(encoder_hidden_states) for att in atts]
        linears = [lin for att in atts for lin in (att.k, att.v)]
        outs = [y for s in range(0, len(linears), ops.T5_PROJ_MAX_GROUP)
                for y in _project(plan, encoder_hidden_states, linears[s:s + ops.T5_PROJ_MAX_GROUP])]
        return [(att._heads(outs[2 * i]), att._heads(outs[2 * i + 1])) for i, att in enumerate(atts)]

    def _call_supported(self, short, dtype, query_length: int, key_length: int, long: bool) -> bool:
        """Whether one attention call has a kernel: by `short`, the short kernel's table, else with `long` the long one's."""
        cfg = self.config
        return short(dtype, cfg.d_kv, cfg.num_heads, query_length, key_length) or (
            long and ops.t5_attention_long_supported(dtype, cfg.d_kv, cfg.num_heads, query_length, key_length))

    def _attention_mode(self, x: Tensor) -> Optional[str]:
        """Which fused attention a forward of x is in, before any length is asked about (module docstring): "train"
        ("hip_train" under grad), "inference" ("hip" or "hip_train" under no_grad, without active dropout), or None."""
        if checked(self, "attention_impl") not in ("hip", "hip_train") or not x.is_cuda:
            return None
        if torch.is_grad_enabled():
            return "train" if self.attention_impl == "hip_train" else None
        return None if self.training and self.config.dropout_rate > 0 else "inference"

    def hip_attention_active(self, x: Tensor, query_length: int, key_length: int,
                             cross_length: Optional[int] = None, cached: bool = False) -> bool:
        """Whether a forward of x with these lengths takes the "hip" path (module docstring).  `cached`: the
        self-attention reads a decode cache, which only the existing kernel does."""
        long = checked(self, "attention_long_impl") == "hip"
        if self._attention_mode(x) != "inference":
            return False
        short = ops.t5_attention_supported
        return self._call_supported(short, x.dtype, query_length, key_length, long and not cached) and (
            cross_length is None or self._call_supported(short, x.dtype, query_length, cross_length, long))

    def hip_train_active(self, x: Tensor, query_length: int, cross_kv: Optional[List[KV]]) -> bool:
        """Whether a forward of x under grad takes the "hip_train" path (module docstring)."""
        long = checked(self, "attention_long_impl") == "hip"
        if self._attention_mode(x) != "train":
            return False
        ok = self._call_supported(ops.t5_attention_bwd_supported, x.dtype, query_length, query_length, long)
        if ok and self.is_decoder:
            ck = cross_kv[0][0]
            ok = ck.shape[0] == x.shape[0] and ck.dtype == x.dtype and self._call_supported(
                ops.t5_attention_bwd_supported, x.dtype, query_length, ck.shape[2], long)
        return ok

    def packed_rows_active(self, x: Tensor, query_length: int, key_bound: int) -> bool:
        """Whether a forward of x can run on packed rows of at most key_bound tokens (module docstring, "Packed rows"): the
        encoder's own rows (query and key bound key_bound), or the decoder's dense self-attention of query_length tokens and
        cross-attention over key_bound.  It takes this forward's fused attention and lengths within the short kernel."""
        cfg, mode = self.config, self._attention_mode(x)
        if mode is None:
            return False
        own = ops.t5_attention_bwd_supported if mode == "train" else ops.t5_attention_supported
        Tq = query_length if self.is_decoder else key_bound  # the packed call's query bound
        return ((not self.is_decoder or own(x.dtype, cfg.d_kv, cfg.num_heads, Tq, Tq))
                and ops.t5_attention_packed_supported(x.dtype, cfg.d_kv, cfg.num_heads, Tq, key_bound))

    def hip_norm_active(self, x: Tensor) -> bool:
        """Whether a forward of x takes the "hip" norm path (module docstring)."""
        return checked(self, "norm_impl") == "hip" and x.is_cuda and ops.t5_add_norm_supported(x.dtype, self.config.d_model)

    def hip_ffn_active(self, x: Tensor) -> bool:
        """Whether a forward of x takes the "hip" feed-forward path (module docstring)."""
        return (checked(self, "ffn_impl") == "hip" and x.is_cuda
                and ops.t5_ffn_supported(x.dtype, self.config.d_model, self.config.d_ff))

    def hip_proj_active(self, x: Tensor) -> bool:
        """Whether the attention projections of a forward of x are grouped "hip" calls (module docstring)."""
        if checked(self, "proj_impl") != "hip" or not x.is_cuda:
            return False
        cfg = self.config
        inner = cfg.num_heads * cfg.d_kv
        if not (ops.t5_proj_supported(x.dtype, cfg.d_model, inner, 3)
                and ops.t5_proj_supported(x.dtype, inner, cfg.d_model)):
            return False
        weights = (lin.weight for blk in self.block for layer in list(blk.layer)[:-1]
                   for att in layer.children() if isinstance(att, T5Attention)
                   for lin in (att.q, att.k, att.v, att.o))
        return all(w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and w.data_ptr() % 16 == 0
                   for w in weights)

    def new_decode_cache(self, steps: int, rows: int, device) -> T5DecodeCache:
        return T5DecodeCache(len(self.block), steps, rows, self.config.num_heads * self.config.d_kv, device)

    def _attention_body(self, inputs_embeds, attention_mask, encoder_hidden_states, encoder_attention_mask,
                        past_key_values, cross_kv, decode_cache, plan: MatmulPlan, packed: Optional[PackedRows] = None,
                        encoder_packed: Optional[PackedRows] = None):
        """The attention body of this forward (module docstring): _HipAttention where it applies, else the operators.
        Packed rows have no operator form: where the fused attention does not apply they raise."""
        R, T = inputs_embeds.shape[0], inputs_embeds.shape[1]
        if packed is not None or encoder_packed is not None:
            rows = packed if packed is not None else encoder_packed
            if self.is_decoder != (packed is None):
                raise ValueError("packed rows: an encoder takes `packed`, a decoder `encoder_packed`")
            if past_key_values is not None or attention_mask is not None or encoder_attention_mask is not None:
                raise ValueError("packed rows take no mask and no operator-format cache (past_key_values): every packed "
                                 "token is valid, and the cached decode step keeps its history in a decode_cache")
            if rows.cu.numel() != rows.batch + 1 or (packed is not None and (R != 1 or T != rows.rows)):
                raise ValueError("packed rows: inputs_embeds is [1, N, d] and cu has batch + 1 entries")
            if packed is not None and decode_cache is not None:
                raise ValueError("packed rows: a decode_cache belongs to the decoder (`encoder_packed`)")
            if packed is None and (rows.batch < 1 or R % rows.batch != 0):
                raise ValueError(f"packed rows: {R} query rows are not a multiple of the {rows.batch} encoder rows")
            if packed is None and torch.is_grad_enabled() and (R != rows.batch or decode_cache is not None):
                raise ValueError("packed rows under grad take one encoder row per query row (beams = 1) and no "
                                 "decode_cache: the beams' cross-attention has no backward")
            if not self.packed_rows_active(inputs_embeds, T, rows.bound):
                raise ValueError('packed rows need the fused attention (attention_impl "hip" / "hip_train", as this '
                                 f"forward would take it) and every length within 256, got bound {rows.bound}")
            if decode_cache is not None and (T != 1 or decode_cache.pos >= decode_cache.steps or R > decode_cache.rows):
                raise ValueError("decode_cache takes one new position per call, within its steps and rows, and no "
                                 "past_key_values or attention_mask")
            if self.is_decoder and cross_kv is None:
                cross_kv = self.cross_kv(encoder_hidden_states, plan)
            return _HipAttention(self, rows.bound if packed is not None else T, None, None, cross_kv, decode_cache,
                                 train=torch.is_grad_enabled(), plan=plan, packed=packed, encoder_packed=encoder_packed)
        if decode_cache is not None or (self.attention_impl != "torch" and past_key_values is None):
            if self.is_decoder and cross_kv is None:
                cross_kv = self.cross_kv(encoder_hidden_states, plan)
            past = 0 if decode_cache is None else decode_cache.pos
            if decode_cache is None and self.hip_train_active(inputs_embeds, T, cross_kv):
                return _HipAttention(self, T, attention_mask, encoder_attention_mask, cross_kv, None, train=True,
                                     plan=plan)
            cross_length = cross_kv[0][0].shape[2] if self.is_decoder else None
            if self.hip_attention_active(inputs_embeds, T, past + T, cross_length, cached=decode_cache is not None):
                if decode_cache is not None and (T != 1 or past_key_values is not None or attention_mask is not None
                                                 or past >= decode_cache.steps or R > decode_cache.rows):
                    raise ValueError("decode_cache takes one new position per call, within its steps and rows, and no "
                                     "past_key_values or attention_mask")
                return _HipAttention(self, T, attention_mask, encoder_attention_mask, cross_kv, decode_cache,
                                     train=False, plan=plan)
            if decode_cache is not None:
                raise ValueError('decode_cache belongs to the "hip" attention path, which is not active here')
        return _OperatorAttention(self, inputs_embeds, attention_mask, encoder_hidden_states, encoder_attention_mask,
                                  past_key_values, cross_kv, plan)

    def _glue(self, layers, fused: bool, p: float, seeds: _Seeds):
        """glue(k, x, y) -> (x + dropout_k(y), norm_k of that sum): what lies between body k - 1 and body k of a
        forward.  k = 0 takes x = None and the input embeddings as y; the last k is the final norm with the stack's
        dropout behind it."""
        norms = [layer.layer_norm for layer in layers] + [self.final_layer_norm]
        last = len(layers)
        if fused:
            def glue(k, x, y):
                return T5AddNormFunction.apply(x, y, norms[k].weight, norms[k].variance_epsilon, p,
                                               p if k == last else 0.0, seeds.glue(k))
        else:
            dropouts = [self.dropout] + [layer.dropout for layer in layers]

            def glue(k, x, y):
                x = dropouts[k](y) if x is None else x + dropouts[k](y)
                normed = norms[k](x)
                return x, self.dropout(normed) if k == last else normed
        return glue

    def forward(self, inputs_embeds: Tensor, attention_mask: Optional[Tensor] = None,
                encoder_hidden_states: Optional[Tensor] = None, encoder_attention_mask: Optional[Tensor] = None,
                past_key_values: Optional[List[KV]] = None, use_cache: bool = False,
                cross_kv: Optional[List[KV]] = None, decode_cache: Optional[T5DecodeCache] = None,
                packed: Optional[PackedRows] = None, encoder_packed: Optional[PackedRows] = None):
        """packed (encoder): inputs_embeds is [1, N, d], the valid tokens of packed.batch rows, and so is the result;
        encoder_packed (decoder): encoder_hidden_states is such a tensor (module docstring, "Packed rows").
        inputs_embeds [R, T, d]; attention_mask [R, past + T] keep-mask (encoder: [R, T]); encoder_attention_mask
        [B, S] keep-mask of the encoder output (B rows, R = B * beams).  Returns the hidden states, and with use_cache
        the per-block self-attention (K, V) including these T positions.  decode_cache ("hip" path, T = 1) holds the
        self-attention history instead of past_key_values: this position's K/V are written into it."""
        self.validate()
        plan = self.matmul_plan(inputs_embeds)  # the images are refreshed here, before the first body
        attention = self._attention_body(inputs_embeds, attention_mask, encoder_hidden_states, encoder_attention_mask,
                                         past_key_values, cross_kv, decode_cache, plan, packed, encoder_packed)
        fused_glue = self.hip_norm_active(inputs_embeds)
        fused_ffn = plan.ffn is not None
        p = float(self.config.dropout_rate) if self.training else 0.0
        layers = [layer for blk in self.block for layer in blk.layer]
        seeds = _Seeds(p, inputs_embeds.device, len(layers) + 1 if fused_glue else 0,
                       len(self.block) if fused_ffn else 0)
        glue = self._glue(layers, fused_glue, p, seeds)

        x, normed = glue(0, None, inputs_embeds)
        k, new_kv = 0, []
        for i, blk in enumerate(self.block):
            out, kv = attention.self_attention(i, blk.layer[0].SelfAttention, normed)
            new_kv.append(kv)
            k += 1
            x, normed = glue(k, x, out)
            del out  # not kept alive through the bodies that follow
            if self.is_decoder:
                k += 1
                x, normed = glue(k, x, attention.cross_attention(i, blk.layer[1].EncDecAttention, normed))
            dense = blk.layer[-1].DenseReluDense
            k += 1
            body = dense.forward_hip(normed, p, seeds.ffn(i), plan) if fused_ffn else dense(normed)
            x, normed = glue(k, x, body)
        return (normed, new_kv) if use_cache else normed


class T5EncoderModel(nn.Module):
    """`shared` table + encoder stack, the layout of HuggingFace's T5EncoderModel (the stack's embed_tokens IS
    `shared`, so both names appear in the state dict)."""

    def __init__(self, config: T5Config) -> None:
        super().__init__()
        self.shared = nn.Embedding(config.vocab_size, config.d_model)
        self.encoder = T5Stack(config, embed_tokens=self.shared)
        nn.init.normal_(self.shared.weight, mean=0.0, std=1.0)

    def forward(self, inputs_embeds: Tensor, attention_mask: Optional[Tensor] = None) -> Tensor:
        return self.encoder(inputs_embeds, attention_mask=attention_mask)


@torch.no_grad()
def init_t5_weights(stack: T5Stack, config: T5Config) -> None:
    """T5's initialisation (initializer_factor 1): normal with the fan-in scales of the mesh-tensorflow T5."""
    d, dk, H = config.d_model, config.d_kv, config.num_heads
    nn.init.normal_(stack.embed_tokens.weight, mean=0.0, std=1.0)
    for blk in stack.block:
        for layer in blk.layer:
            layer.layer_norm.weight.fill_(1.0)
            att = getattr(layer, "SelfAttention", None) or getattr(layer, "EncDecAttention", None)
            if att is not None:
                att.q.weight.normal_(0.0, (d * dk) ** -0.5)
                att.k.weight.normal_(0.0, d ** -0.5)
                att.v.weight.normal_(0.0, d ** -0.5)
                att.o.weight.normal_(0.0, (H * dk) ** -0.5)
                if att.has_relative_attention_bias:
                    att.relative_attention_bias.weight.normal_(0.0, d ** -0.5)
            else:
                layer.DenseReluDense.wi.weight.normal_(0.0, d ** -0.5)
                layer.DenseReluDense.wo.weight.normal_(0.0, config.d_ff ** -0.5)
    stack.final_layer_norm.weight.fill_(1.0)
