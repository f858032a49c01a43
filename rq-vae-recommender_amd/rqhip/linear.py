"""Kernel selection for the bias-free Linear(+ReLU) layers of the MLPs.  Which kernel a layer's forward, data gradient and weight
gradient take is decided in ONE place, `plan_layer`: a function of row count, widths and switches.  The whole-stack autograd node of
modules/encoder.py (`_MLPStack`) and the per-layer path (`forward` / `input_grad` / `weight_grad` / `backward` here, run by the
per-layer Function and the registered operators of rqhip/torch_ops.py) both dispatch on it, which is why the tests can compare them
bit for bit; the two places where they decide differently are arguments of `plan_layer` (`relu`, `stack_jobs`).

The large layers run on the 16-bit matrix cores with fp32's accuracy (csrc/gemm_split.hip, csrc/wgrad_split.hip).  Round 4's
product arithmetic is `f16x2`: every row (column, for the weight gradients) is scaled by an exact power of two and split into
two fp16 pieces, three piece products per product.  The scales are the maxima of the rows / columns of the operand, which the
kernel that WROTE the operand emits from its epilogue (`Scales`, handed from layer to layer by modules/encoder.py:_MLPStack);
a caller that has none gets them from one `ops.maxima` pass -- same maxima, same exponents, same result bits either way.  (One exception:
when the reconstruction loss's upstream gradient is not the announced 1 / B -- `ops.recon_rescale_rows` -- rows that were scaled DOWN leave
the column maxima of that gradient too large: still a valid scale, one low-order bit of the fp16 low piece per binade of overestimate,
and not the bits a fresh maxima pass would give.  No shipped training loop takes that path: the loss is a mean.)
`use_arith("bf16x3")` keeps round 3's three-piece bf16 kernels for A/B (bench.py --mlp split6).

What the host side of a step tells itself across autograd nodes, and how: the maxima that came with a stack's input (`attached_scales`) and
whether the stack may park its weight gradients are ARGUMENTS of `_MLPStack.apply`; weight-gradient jobs are `WgradJob`s, launched by
`launch_wgrads` and parked in `wgrad_queue` (the contract: `WgradQueue`); the one remaining call-order slot is `handoff_grad`, which
carries pointer, shape and version of the gradient it speaks about."""
from enum import IntEnum
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _lib, ops

# ---- the large activation GEMMs on the matrix cores (csrc/gemm_split.hip) -------------------------------------------------------
# Measured at 100 000 rows against the tuned library fp32 GEMM of the same layer (tools/bench_gemm_split.py, and in the
# step: profiles/r04_*): every supported forward and data gradient is faster.  Small batches are launch-bound and stay with
# the library.
SPLIT_MIN_ROWS = 4096
_SPLIT_GEMMS = True
_ARITH = ops.F16X2
_FP32 = -1   # no split kernels at all: library fp32 GEMMs, fp32-MFMA weight gradients (round 2's step, bench.py --mlp library)
_ARITH_NAMES = {"f16x2": ops.F16X2, "bf16x3": ops.BF16X3, "fp32": _FP32}


def use_split_gemms(on: bool = True) -> bool:
    """Route the large activation GEMMs through csrc/gemm_split.hip (default) or the library (A/B: tools/ab_step.py).
    Returns the previous setting."""
    global _SPLIT_GEMMS
    before, _SPLIT_GEMMS = _SPLIT_GEMMS, bool(on)
    return before


def use_arith(name: str) -> str:
    """"f16x2" (two fp16 pieces under exact power-of-two scales, three products: the product path), "bf16x3" (round 3: three
    bf16 pieces, six products) or "fp32" (round 2: library fp32 GEMMs and the oracle-ordered fp32-MFMA weight gradients).
    Returns the previous setting's name."""
    global _ARITH
    before = arith_name()
    _ARITH = _ARITH_NAMES[name]
    return before


def arith_name() -> str:
    return next(k for k, v in _ARITH_NAMES.items() if v == _ARITH)


def f16() -> bool:
    return _ARITH == ops.F16X2


class Scales:
    """What the fp16 kernels need to know about an operand [M, N]: `rows` int32 [parts, M] (a row's largest |value| is the
    maximum over the parts, bit patterns), `cols` int32 [N]; either may be missing (None) until someone needs it."""
    __slots__ = ("rows", "cols")

    def __init__(self, rows: Optional[Tensor] = None, cols: Optional[Tensor] = None):
        self.rows, self.cols = rows, cols


# ---- maxima that come with the data ----------------------------------------------------------------------------------------------
# The largest |value| of an item's feature row is a property of the ITEM: the HBM-resident item matrix (data/processed.py:ItemData)
# computes it once per corpus and hands it out with every batch it gathers (`attach_scales`), and the stack that reads the batch takes
# it from there instead of running rqhip_maxima over the batch again (82 us of a 2.86 ms step at 100 000 x 768).  The column maxima the
# first layer's weight gradient wants are replaced by the corpus-wide ones, an upper bound for every batch (costs low-order bits of
# entries more than 2^16 below their column's corpus maximum only; same rule as a masked gradient under unmasked maxima).
def attach_scales(t: Tensor, rows: Optional[Tensor], cols: Optional[Tensor]) -> Tensor:
    """Remember on the tensor OBJECT `t` [M, N] the bit patterns of its row maxima (`rows`: int32 [1, M]) and of (upper bounds of)
    its column maxima (`cols`: int32 [N]); views / copies of `t` do not inherit them."""
    t._rq_scales = Scales(rows, cols)
    return t


def attached_scales(t: Tensor) -> Optional[Scales]:
    sc = getattr(t, "_rq_scales", None)
    if sc is None:
        return None
    ok_r = sc.rows is None or (sc.rows.dtype == torch.int32 and sc.rows.dim() == 2 and sc.rows.shape[1] == t.shape[0] and sc.rows.device == t.device)
    ok_c = sc.cols is None or (sc.cols.dtype == torch.int32 and tuple(sc.cols.shape) == (t.shape[1],) and sc.cols.device == t.device)
    return Scales(sc.rows if ok_r else None, sc.cols if ok_c else None)


# ---- zeroed int32 slices for column maxima ---------------------------------------------------------------------------------------------
# Every kernel that emits column maxima accumulates them with atomic maxima into a buffer the caller zeroed; a training step at 100 000
# rows asked for six such buffers, each a `torch.zeros` = one 4 us fill launch (28 us of a 2.7 ms step).  They are cut from a pool that
# is zeroed ONCE (64 K words = one fill per ~20 steps); a slice is handed out once and never reused, an exhausted pool is replaced (its
# slices live on as long as somebody holds them).  Under hipGraph capture a replay would meet non-zero slices: there, plain torch.zeros.
_ZERO_POOL = {}
_ZERO_POOL_WORDS = 1 << 16
_TRIMS = True


def use_step_trims(on: bool = True) -> bool:
    """A/B switch (bench.py --no-trims) for round 6's launch-overhead trims: pooled zero arenas (zeros_i32), the duplicate statistic on a
    side stream (modules/rqvae.py), the many-workgroup loss means (ops.loss_means).  Returns the previous setting."""
    global _TRIMS
    before, _TRIMS = _TRIMS, bool(on)
    return before


def trims_on() -> bool:
    return _TRIMS


def zeros_i32(n: int, device) -> Tensor:
    """A zeroed int32 [n] tensor nobody else holds (a 16-byte aligned slice of the device's pool; see above)."""
    if n <= 0:
        return torch.zeros((0,), dtype=torch.int32, device=device)
    if not _TRIMS or n > _ZERO_POOL_WORDS // 4 or torch.cuda.is_current_stream_capturing():
        return torch.zeros((n,), dtype=torch.int32, device=device)
    key = (torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device(),
           torch.cuda.current_stream(device).cuda_stream)     # (a pool belongs to the stream its fill ran on)
    pool = _ZERO_POOL.get(key)
    need = (n + 3) // 4 * 4
    if pool is None or pool[1] + need > _ZERO_POOL_WORDS:
        pool = [torch.zeros((_ZERO_POOL_WORDS,), dtype=torch.int32, device=device), 0]
        _ZERO_POOL[key] = pool
    out = pool[0][pool[1]:pool[1] + n]
    pool[1] += need
    return out


def col_slices(widths: Sequence[int], device) -> List[Optional[Tensor]]:
    """One zeroed int32 [n] slice per width n > 0 (None for 0), all cut from one `zeros_i32` arena: where the epilogues of a stack's
    GEMMs put the column maxima of what they store."""
    arena = zeros_i32(sum(widths), device) if any(widths) else None
    return [arena[sum(widths[:i]):sum(widths[:i + 1])] if n else None for i, n in enumerate(widths)]


_GRAD_HANDOFF: List[Optional[tuple]] = [None]


def handoff_grad(g: Tensor, sc: Scales) -> None:
    """The NEXT `_MLPStack.backward` that receives `g` (same storage, same shape, not written since) as its upstream gradient may take it
    as already masked by its last layer's ReLU, with these maxima (set by the backward of modules/rqvae.py's seam node, whose epilogue did
    both).  The version is part of the proof: a second consumer of the hidden activation makes autograd's input buffer add its gradient
    into `g` in place -- same pointer, another version, and a sum that is neither masked nor under these maxima."""
    _GRAD_HANDOFF[0] = (g.data_ptr(), tuple(g.shape), g._version, sc)


def take_grad_handoff(g: Tensor) -> Optional[Scales]:
    slot, _GRAD_HANDOFF[0] = _GRAD_HANDOFF[0], None     # one shot: whoever asks next clears it, match or not
    if slot is not None and slot[:3] == (g.data_ptr(), tuple(g.shape), g._version):
        return slot[3]
    return None


def ensure_scales(a: Tensor, sc: Optional[Scales], rows: bool, cols: bool) -> Scales:
    """`sc` with the requested maxima present: what is missing is computed by ONE pass over `a` (rqhip_maxima)."""
    sc = sc if sc is not None else Scales()
    need_r, need_c = rows and sc.rows is None, cols and sc.cols is None
    if need_r or need_c:
        r, c, _ = ops.maxima(a, rows=need_r, cols=need_c)
        if need_r:
            sc.rows = r
        if need_c:
            sc.cols = c
    return sc


def _wide(n_cols: int) -> bool:
    """Layers of 128 (mod 128) output columns: 256-column tiles (the product kernel) or, for 128 (mod 256) columns, the staged
    loop's 128-column tile.  Round 3 left the latter to the library (HBM-bound shapes, measured level: 100 000 x 256 -> 128
    forward 58 us vs 67, its data gradient 59 vs 56); with the f16x2 arithmetic, maxima from the epilogues and the transposing
    epilogue the step is 2 % faster with them on the split kernel (3.06 -> 2.99 ms, bench.py --no-narrow for the A/B)."""
    return n_cols % 256 == 0 or (_NARROW and n_cols % 128 == 0)


_NARROW = True


def use_narrow_tiles(on: bool = True) -> bool:
    """A/B switch (bench.py --no-narrow): layers of 128 (mod 256) output columns through the split kernel's 128-column tile as well."""
    global _NARROW
    before, _NARROW = _NARROW, bool(on)
    return before


def wgrad_f16_ok(n_out: int, n_in: int, rows: int = SPLIT_MIN_ROWS) -> bool:
    """Does the weight gradient of an [n_out, n_in] layer over `rows` batch rows run on the fp16 split kernel (and therefore
    want column maxima)?  The shapes csrc/wgrad_split.hip tiles: both multiples of 128, one of them of 256 -- and batches of
    4096 rows and more: below that a step is launch-bound, and the maxima passes / zeroed arenas the scales need are launches
    (batch 640: 71 device activities per step with them, 1.55 ms; the fused-mask kernels of csrc/wgrad.hip need none)."""
    return bool(f16() and rows >= SPLIT_MIN_ROWS and n_out % 128 == 0 and n_in % 128 == 0 and (n_out % 256 == 0 or n_in % 256 == 0))


_WGRAD_BATCH = True


def use_wgrad_batch(on: bool = True) -> bool:
    """A/B (round 6): at split-kernel batch sizes the weight gradients of an MLP stack's 256 x 256-tiled layers in ONE launch
    (rqhip_linear_wgrad_f16_batch: half the partial-block traffic of two launches; default) or one launch per layer.  Returns the
    previous setting."""
    global _WGRAD_BATCH
    before, _WGRAD_BATCH = _WGRAD_BATCH, bool(on)
    return before


# ---- weight-gradient jobs: one record, one launcher, one waiting list -------------------------------------------------------------------
class WgradJob(NamedTuple):
    """dW [n_out, n_in] = g^T x of one layer: `w` (for its shape), `g` [M, n_out] already masked by the layer's ReLU, `x` [M, n_in], the
    column maxima of both for the fp16 split kernel (None, None: a job of the job-table kernel, batches below 4096 rows), `sink`: the
    tensor to write (the parameter's slice of a flat gradient buffer) or None = a fresh one."""
    w: Tensor
    g: Tensor
    x: Tensor
    g_cols: Optional[Tensor]
    x_cols: Optional[Tensor]
    sink: Optional[Tensor]


def _launch_group(jobs: List[WgradJob]) -> List[Tensor]:
    if jobs[0].g_cols is None:
        return ops.linear_wgrad_jobs([(j.g, j.x) for j in jobs], outs=[j.sink for j in jobs])
    if len(jobs) >= 2 and ops.linear_wgrad_f16_batch_ranges(jobs[0].g.shape[0], [tuple(j.w.shape) for j in jobs]) >= 1:
        return ops.linear_wgrad_f16_batch([(j.g, j.x, j.g_cols, j.x_cols) for j in jobs], outs=[j.sink for j in jobs])
    return [weight_grad(j.g, None, j.x, j.w, out=j.sink, want_masked=False, g_scales=Scales(None, j.g_cols), x_scales=Scales(None, j.x_cols),
                        premasked=True)[0] for j in jobs]


def launch_wgrads(jobs: List[WgradJob], waited: Sequence[WgradJob] = ()) -> List[Tensor]:
    """Launch `jobs` and return their dW in order.  fp16 jobs first: the layers tiled 256 x 256 together, the half-tiled ones (128 x 256 /
    256 x 128) together, at most 4 per launch, one batched launch where the plan allows, else per layer; then the job-table jobs, at most
    ops.WGRAD_JOBS_MAX per launch.  `waited`: an earlier stack's jobs (`WgradQueue.take`), launched in the same groups as `jobs` when every
    one of `jobs` has a sink and both have the same row count and device -- a batched launch cuts its layers into a number of row ranges
    that depends on which layers share it, so the grouping decides result bits -- else on their own, first."""
    if waited and not (jobs and all(j.sink is not None for j in jobs)
                       and (waited[0].g.shape[0], waited[0].g.device) == (jobs[0].g.shape[0], jobs[0].g.device)):
        launch_wgrads(waited)
        waited = ()
    todo = [*waited, *jobs]
    dws: List[Optional[Tensor]] = [None] * len(todo)
    groups = ([], [], [])       # indices of: fp16 jobs tiled 256 x 256, fp16 jobs half-tiled, job-table jobs
    for i, j in enumerate(todo):
        groups[2 if j.g_cols is None else 0 if (j.w.shape[0] % 256 == 0 and j.w.shape[1] % 256 == 0) else 1].append(i)
    for idx, per_launch in zip(groups, (4, 4, ops.WGRAD_JOBS_MAX)):
        for c in range(0, len(idx), per_launch):
            part = idx[c:c + per_launch]
            for i, dw in zip(part, _launch_group([todo[i] for i in part])):
                dws[i] = dw
    return dws[len(waited):]


_CROSS_STACK = True


def use_wgrad_cross_stack(on: bool = True) -> bool:
    """A/B (round 6): the decoder's batched weight gradients wait for the encoder's launch (default) or are launched per stack."""
    global _CROSS_STACK
    before, _CROSS_STACK = _CROSS_STACK, bool(on)
    return before


class WgradQueue:
    """Weight-gradient jobs of one stack that wait for a later stack's launch in the same backward pass (`wgrad_queue`, the only instance).

    Why: the decoder's backward runs before the encoder's.  At split-kernel batches one rqhip_linear_wgrad_f16_batch over both stacks' layers
    (16 tiles x 16 row ranges instead of twice 8 x 32) beats one per stack; below 4096 rows one job-table launch serves both stacks (also
    inside a hipGraph capture: the engine's callback runs inside the captured region like everything else of the step).

    Who may park: a `_MLPStack` node whose module is tagged `_defer_wgrads` (RqVae's decoder), when nothing waits already and `may_park`
    holds -- one rank (with several the decoder's gradients go on the wire under the encoder's backward: FlatGradReducer.boundary_hook), the
    A/B switches on, every job with a slice of the flat gradient buffer to land in (rqhip/dist.py:claim_grad_sink), no hook on a weight.
    Who launches: the next `_MLPStack.backward` of the pass (`take`, then `launch_wgrads(own, waited)`), or the callback the autograd engine
    runs when the pass ends (an encoder without gradients, a stack used on its own) -- on the stream the parking backward ran on, which
    need not be current on the thread that called backward().
    What the parked dW is until then: the node has returned an alias of the sink, autograd has made it `.grad`, and it still holds the
    PREVIOUS step's values; the launch fills it before anything later on the stream reads it.  Whatever reads a gradient between the node
    and the launch -- a tensor hook, a post-accumulate-grad hook -- would see stale values, hence no parking for a hooked weight.
    A pass that ended in an exception leaves its jobs here: `clear` (RqVae.forward) drops them."""

    def __init__(self) -> None:
        self._jobs: List[WgradJob] = []
        self._stream = None

    def waiting(self) -> bool:
        return bool(self._jobs)

    def may_park(self, jobs: List[WgradJob]) -> bool:
        from . import dist as _dist
        kind_ok = _WGRAD_JOBS if jobs[0].g_cols is None else (_WGRAD_BATCH and not torch.cuda.is_current_stream_capturing())
        return bool(_CROSS_STACK and kind_ok and _dist.world_size() == 1 and all(j.sink is not None for j in jobs)
                    and not any(j.w._backward_hooks or j.w._post_accumulate_grad_hooks for j in jobs))

    def park(self, jobs: List[WgradJob]) -> None:
        if not self._jobs:
            torch.autograd.Variable._execution_engine.queue_callback(self._flush)
            self._stream = torch.cuda.current_stream()
        self._jobs.extend(jobs)

    def take(self) -> List[WgradJob]:
        jobs, self._jobs = self._jobs, []
        return jobs

    def clear(self) -> None:
        self._jobs = []

    def _flush(self) -> None:
        jobs, st = self.take(), self._stream
        if jobs and st is not None and st != torch.cuda.current_stream(st.device):
            with torch.cuda.stream(st):
                launch_wgrads(jobs)
        elif jobs:
            launch_wgrads(jobs)


wgrad_queue = WgradQueue()


_WGRAD_JOBS = True


def use_wgrad_jobs(on: bool = True) -> bool:
    """Batches below the split kernels' 4096 rows -- the sizes the reference's gin files train with -- take the job-table
    weight-gradient kernel (csrc/wgrad_jobs.hip: every layer of an MLP stack in one launch, no row ranges, no reduction launches;
    default on).  Off: round 4's per-layer kernels (A/B: tools/bench_small_batch.py --no-jobs).  Returns the previous setting."""
    global _WGRAD_JOBS
    before, _WGRAD_JOBS = _WGRAD_JOBS, bool(on)
    return before


def wgrad_jobs_ok(rows: int, shapes) -> bool:
    """Do the weight gradients of layers `shapes` = [(n_out, n_in), ...] over `rows` batch rows run as ONE job-table launch?"""
    shapes = list(shapes)
    return bool(_WGRAD_JOBS and _ARITH != _FP32 and 0 < rows < SPLIT_MIN_ROWS and 0 < len(shapes) <= ops.WGRAD_JOBS_MAX
                and all(ops.linear_wgrad_jobs_supported(n, k) for n, k in shapes))


_WIDE_TILES = False
_WIDE_MIN_RED = 512


def use_wide_tiles(on: bool = True) -> bool:
    """A/B arm, default OFF (round 6): layers of 512 (mod 512) output columns with a reduction of 512 and more on
    full-output-width tiles (128 x 512, 8 waves, ONE workgroup per CU: a strip of A is fetched and split once per row tile) instead of
    two 128 x 256 tiles of two workgroups per CU.  Same result bits; HBM traffic and VALU work per matrix instruction fall as intended
    and the kernels get 4-6 % SLOWER inside the step (768 -> 512 forward 258 -> 273 us, its data gradient 269 -> 280 us:
    profiles/r06_gemm_wide_ab.txt) -- eight waves behind one barrier idle together, two independent workgroups do not.
    bench.py --wide-tiles, tools/gemm_wide_ab.py.  Returns the previous setting."""
    global _WIDE_TILES
    before, _WIDE_TILES = _WIDE_TILES, bool(on)
    return before


_TINY_TILES = False
_ROWS_WITH_COLS = True     # (the note in `gemm` below; A/B on one box: 2.5385 vs 2.5456 ms, profiles/r06_step_ab.txt)
_STATIC_TILES = True


def use_static_tiles(on: bool = True) -> bool:
    """A/B (round 6): the product GEMM's tiles dealt statically (workgroup b: tiles b, b + grid, ...; default) or handed out by the
    atomic dispenser of rounds 4-5.  Returns the previous setting."""
    global _STATIC_TILES
    before, _STATIC_TILES = _STATIC_TILES, bool(on)
    return before


def use_tiny_tiles(on: bool = True) -> bool:
    """A/B (round 6, neutral in the step, off by default): the product GEMM's leftover behind the whole rounds of 128-row tiles as 32-row
    tiles where the launch plan prices them cheaper, instead of round 5's plan (64-row leftover tiles / all big).  Returns the previous
    setting."""
    global _TINY_TILES
    before, _TINY_TILES = _TINY_TILES, bool(on)
    return before


def _tile_code(n_cols: int, n_red: int, epilogue: int) -> int:
    """rqhip_gemm_args.tile_rows for a layer: -5 selects the 128 x 512 tile (csrc/gemm_split.hip), -9 allows 32-row leftover tiles, -12 the atomic tile dispenser, 0 the default."""
    if _WIDE_TILES and f16() and n_cols % 512 == 0 and n_red >= _WIDE_MIN_RED and epilogue != _lib.EPI_RECON:
        return -5
    if not _STATIC_TILES:
        return -12
    return -9 if _TINY_TILES else 0


# ---- the 32-wide layers either side of the quantiser (the RQ <-> MLP seam) ------------------------------------------------------------
# The encoder's last Linear (128 -> 32) and the decoder's first (32 -> 128), forward and data gradient, run on csrc/rq_forward.hip's seam
# kernel (rqhip_rq_seam): every output is ONE fp32 FMA chain over the input features on the fp32 matrix pipe -- no library call, the ReLU /
# ReLU backward and the maxima the neighbouring split kernels scale by in the same launch, and the same bits in the fused launch
# RqVae.forward uses (modules/rqvae.py), which is this kernel with the quantisation levels switched on.  Batches of 4096 rows and more:
# every output is a 64- or 16-deep chain of dependent fp32 matrix instructions over 32 rows at a time -- at the reference's batch 640, 20
# such chains on 20 SIMDs, 9.3 us per launch against 4.6-5.9 us for the library's 16 x 16 tiles (profiles/r06_seam.txt); see SMALL below.
_CHAIN = True
CHAIN_D, CHAIN_H = 32, ops.SEAM_H


def use_chain_gemms(on: bool = True) -> bool:
    """The 128 <-> 32 layers on the seam kernel (default) or on the library / split kernels as in round 5 (A/B: bench.py --no-seam).
    Returns the previous setting."""
    global _CHAIN
    before, _CHAIN = _CHAIN, bool(on)
    return before


def chain_gemms_on() -> bool:
    return _CHAIN


def chain_forward(x: Tensor, w: Tensor, relu: bool, want_rows: bool = False, col_out: Optional[Tensor] = None):
    """(y, Scales of y) of y = [relu](x w^T) for a seam layer (`plan_layer`: SEAM_IN / SEAM_OUT; a ReLU only behind the 32 -> 128 layer)."""
    x = x if x.is_contiguous() else x.contiguous()
    if tuple(w.shape) == (CHAIN_D, CHAIN_H):
        assert not relu
        return ops.rq_seam(h=x, w_in=w.detach()).res0, Scales()
    r = ops.rq_seam(res0=x, w_out=w.detach(), epilogue=_lib.EPI_RELU if relu else _lib.EPI_STORE, want_row_max=want_rows and f16(),
                    col_max_out=col_out if f16() else None)
    return r.out, Scales(r.out_row_max, col_out if f16() else None)


def chain_input_grad(g: Tensor, w: Tensor, *, g_mask: Optional[Tensor] = None, out_mask: Optional[Tensor] = None, want_rows: bool = False,
                     col_out: Optional[Tensor] = None):
    """(gx, Scales of gx) of gx = g' w for a seam layer with weight w [n_out, n_in]; g' = g where g_mask > 0 (the layer's own ReLU
    backward, applied on load: 32 -> 128 layers only); gx is kept where out_mask > 0 (the ReLU backward of the layer below, in the
    epilogue: 128 -> 32 layers only)."""
    g = g if g.is_contiguous() else g.contiguous()
    if tuple(w.shape) == (CHAIN_H, CHAIN_D):       # layer 32 -> 128, w [128, 32]: gx [B, 32] = g' [B, 128] . w
        assert out_mask is None
        return ops.rq_seam(h=g, h_mask=g_mask, w_in=w.detach(), w_in_transposed=True).res0, Scales()
    assert g_mask is None                 # layer 128 -> 32, w [32, 128]: gx [B, 128] = g [B, 32] . w
    r = ops.rq_seam(res0=g, w_out=w.detach(), w_out_transposed=True, epilogue=_lib.EPI_MASK if out_mask is not None else _lib.EPI_STORE,
                    out_mask=out_mask, want_row_max=want_rows and f16(), col_max_out=col_out if f16() else None)
    return r.out, Scales(r.out_row_max, col_out if f16() else None)


# ---- batches below 4096 rows: the layers' forward and data gradient on csrc/mlp_small.hip (rqhip_linear_small) -----------------------
# Exact fp32 on the fp32 matrix instruction, the ReLU / the ReLU backward of the layer below in the epilogue: at the reference's batch
# sizes (640 / 64 rows) a training step has no library GEMM and no threshold_backward launch left (rounds 1-5: 16 + 6 of its 39 launches).
_SMALL = True


def use_small_kernels(on: bool = True) -> bool:
    """rqhip_linear_small below 4096 rows (default) or the library GEMMs as in round 5 (A/B: tools/bench_small_batch.py --no-small).
    Returns the previous setting."""
    global _SMALL
    before, _SMALL = _SMALL, bool(on)
    return before


def small_forward(x: Tensor, w: Tensor, relu: bool) -> Tensor:
    """[relu](x w^T) on rqhip_linear_small (`plan_layer`: SMALL)."""
    return ops.linear_small(x, w.detach(), epilogue=_lib.EPI_RELU if relu else _lib.EPI_STORE)


def small_input_grad(g: Tensor, w: Tensor, below: Optional[Tensor] = None) -> Tensor:
    """g w for w [n_out, n_in], kept where `below` [M, n_in] > 0 (the ReLU backward of the layer below) when given."""
    return ops.linear_small(g, w.detach(), w_kn=True, epilogue=_lib.EPI_MASK if below is not None else _lib.EPI_STORE, aux=below)


# ---- the plan: which kernel a layer's forward, data gradient and weight gradient take ---------------------------------------------------
class Route(IntEnum):
    NONE = 0                # this direction is not computed (nobody wants the gradient)
    LIBRARY = 1             # the library's fp32 GEMM (widths no kernel tiles, operands no kernel takes, the strict-fp32 arm)
    SPLIT = 2               # csrc/gemm_split.hip: 4096 rows and more, 128 (mod 128) output columns
    SEAM_IN = 3             # csrc/rq_forward.hip's seam kernel, a 128 -> 32 product (the rows enter through its input GEMM)
    SEAM_OUT = 4            # ... a 32 -> 128 product (the rows leave through its output GEMM, which can emit maxima)
    SMALL = 5               # csrc/mlp_small.hip: below 4096 rows
    F16_SPLIT = 6           # weight gradient on csrc/wgrad_split.hip, one launch for the layer
    F16_SPLIT_BATCHED = 7   # ... and the layer may wait for a launch it shares with other layers (`launch_wgrads`)
    FP32_MFMA = 8           # weight gradient on csrc/wgrad.hip (round 3's kernels; oracle-ordered in the strict-fp32 arm)
    JOBS = 9                # weight gradient on csrc/wgrad_jobs.hip: below 4096 rows


class LayerPlan(NamedTuple):
    fwd: Route
    dgrad: Route
    wgrad: Route

    @property
    def wgrad_f16(self) -> bool:        # the fp16 split kernel: the weight gradient wants column maxima of both its operands
        return self.wgrad in (Route.F16_SPLIT, Route.F16_SPLIT_BATCHED)


def dense_f32(t: Tensor) -> bool:
    """The operand form the kernels take: a 2-D fp32 ROCm tensor, contiguous, rows 16-byte aligned."""
    return bool(t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous() and t.data_ptr() % 16 == 0)


def _gemm_route(rows: int, n_cols: int, n_red: int, seam: bool, small: bool) -> Route:
    """out [rows, n_cols] = a [rows, n_red] . B, a forward or a data gradient; seam / small: those kernels may be used."""
    if rows >= SPLIT_MIN_ROWS:
        if seam and (n_cols, n_red) == (CHAIN_D, CHAIN_H):
            return Route.SEAM_IN
        if seam and (n_cols, n_red) == (CHAIN_H, CHAIN_D):
            return Route.SEAM_OUT
        if _SPLIT_GEMMS and _ARITH != _FP32 and _wide(n_cols) and ops.gemm_split_supported(n_cols, n_red):
            return Route.SPLIT
    elif small and _ARITH != _FP32 and n_cols % 32 == 0 and n_red % 32 == 0:     # (strict fp32 means "library")
        return Route.SMALL
    return Route.LIBRARY


def plan_layer(rows: int, n_out: int, n_in: int, *, relu: bool, operands_aligned: bool, weight_ok: bool = True,
               need_dgrad: bool = True, need_wgrad: bool = True, stack_jobs: bool = False) -> LayerPlan:
    """The kernels of a bias-free Linear n_in -> n_out over `rows` batch rows under the module's switches (ints and bools only: testable
    without a device).  operands_aligned: activations and gradients have 16-byte aligned rows, which the seam kernel and rqhip_linear_small
    need; weight_ok: the weight is `dense_f32` (rqhip_linear_small alone reads it as it lies).  The two places where the stack node and the per-layer path decide differently, kept as they are:
    relu -- the layer is followed by a ReLU.  The seam kernel has no ReLU behind its input GEMM, so a 128 -> 32 layer with one stays off
      it.  The stack says so for both directions; the per-layer `input_grad` is not told about the ReLU and passes False, so there the
      data gradient of such a layer still takes the seam kernel.  (No shipped configuration has that layer.)
    stack_jobs -- the caller is a stack whose layers TOGETHER pass `wgrad_jobs_ok`: one job-table launch for all of them, including
      layers csrc/wgrad.hip does not tile (64 x 64), which the per-layer path, asking that kernel's shape rule first, leaves to the
      library."""
    if rows <= 0:
        return LayerPlan(Route.LIBRARY, Route.LIBRARY if need_dgrad else Route.NONE, Route.LIBRARY if need_wgrad else Route.NONE)
    seam = _CHAIN and operands_aligned and not (relu and (n_out, n_in) == (CHAIN_D, CHAIN_H))
    small = _SMALL and operands_aligned and weight_ok
    fwd = _gemm_route(rows, n_out, n_in, seam, small)
    dgrad = _gemm_route(rows, n_in, n_out, seam, small) if need_dgrad else Route.NONE
    if not need_wgrad:
        wgrad = Route.NONE
    elif stack_jobs:
        wgrad = Route.JOBS
    elif not ops.linear_wgrad_supported(n_out, n_in):
        wgrad = Route.LIBRARY
    elif wgrad_jobs_ok(rows, [(n_out, n_in)]):
        wgrad = Route.JOBS
    elif wgrad_f16_ok(n_out, n_in, rows):
        wgrad = Route.F16_SPLIT_BATCHED if _WGRAD_BATCH else Route.F16_SPLIT
    else:
        wgrad = Route.FP32_MFMA
    return LayerPlan(fwd, dgrad, wgrad)


def images(jobs: List[Tuple[Tensor, bool]]) -> List[Tensor]:
    """The weight images of `jobs` = [(w, transpose), ...] in the current arithmetic, one launch.  Rebuilt at EVERY forward:
    a first version cached an image per `w._version` -- and trained on stale weights: the fused AdamW update (and any
    `w.data` write) does not bump the version counter.  The images of an MLP's forward and data-gradient GEMMs are built
    together when its forward starts (weights cannot change between a forward and its backward); inside a hipGraph capture
    the build is part of the graph, as it has to be."""
    return ops.weight_images([(w.detach(), tr) for w, tr in jobs], _ARITH)


def planes(w: Tensor, transpose: bool) -> Tensor:
    return images([(w, transpose)])[0]


def gemm(a: Tensor, image: Tensor, n_cols: int, *, epilogue: int = _lib.EPI_STORE, aux: Optional[Tensor] = None,
         row_scale: float = 0.0, a_scales: Optional[Scales] = None, want_rows: bool = False,
         col_out: Optional[Tensor] = None):
    """One split GEMM in the current arithmetic.  Returns (C, loss_rows, Scales of C): the row maxima of `a` come from
    `a_scales` or from a pass; the Scales of C hold the row maxima when `want_rows` and `col_out` (a zeroed int32 [n_cols]
    slice that receives the column maxima) when given -- both only in the f16x2 arithmetic (the bf16 path needs none)."""
    rows_in = ensure_scales(a, a_scales, True, False).rows if f16() else None
    # (a launch that emits column maxima also emits row maxima, wanted or not: the kernel's straight-line epilogue is the form with both --
    # csrc/gemm_split.hip:gs_epilogue -- and the general loop costs such a launch ~10 %; the extra [column tiles, M] words are dropped)
    c, loss_rows, crm = ops.gemm_split_ex(a, image, n_cols, arith=_ARITH, epilogue=epilogue, aux=aux, row_scale=row_scale,
                                          a_row_max=rows_in, want_row_max=(want_rows or (col_out is not None and _ROWS_WITH_COLS)) and f16(),
                                          col_max_out=col_out if f16() else None, tile_rows=_tile_code(n_cols, a.shape[1], epilogue))
    return c, loss_rows, Scales(crm if want_rows else None, col_out if f16() else None)


def input_grad(g: Tensor, w: Tensor, *, g_scales: Optional[Scales] = None, image: Optional[Tensor] = None) -> Tensor:
    """g [M, N] . w [N, K] on the kernel `plan_layer` names (the split kernel with the image of w^T)."""
    g = g if g.is_contiguous() else g.contiguous()
    # relu=False: nobody tells this function whether a ReLU follows the layer -- the first difference in `plan_layer`'s docstring
    route = plan_layer(g.shape[0], w.shape[0], w.shape[1], relu=False, operands_aligned=True, weight_ok=dense_f32(w),
                       need_wgrad=False).dgrad if dense_f32(g) else Route.LIBRARY
    if route in (Route.SEAM_IN, Route.SEAM_OUT):
        return chain_input_grad(g, w)[0]
    if route == Route.SPLIT:
        return gemm(g, image if image is not None else planes(w, True), w.shape[1], a_scales=g_scales)[0]
    if route == Route.SMALL:
        return small_input_grad(g, w)
    return g.mm(w)


def forward(x: Tensor, w: Tensor, relu: bool, zero_bias: Tensor = None) -> Tensor:
    """relu(x w^T) or x w^T on the kernel `plan_layer` names; the library GEMM has the ReLU in the hipBLASLt epilogue."""
    route = plan_layer(x.shape[0], w.shape[0], w.shape[1], relu=relu, operands_aligned=True, weight_ok=dense_f32(w),
                       need_dgrad=False, need_wgrad=False).fwd if dense_f32(x) else Route.LIBRARY
    if route in (Route.SEAM_IN, Route.SEAM_OUT):
        return chain_forward(x, w, relu)[0]
    if route == Route.SPLIT:
        return gemm(x, planes(w, False), w.shape[0], epilogue=_lib.EPI_RELU if relu else _lib.EPI_STORE)[0]
    if route == Route.SMALL:
        return small_forward(x, w, relu)
    return library_forward(x, w, relu, zero_bias)


def library_forward(x: Tensor, w: Tensor, relu: bool, zero_bias: Tensor = None) -> Tensor:
    if relu:
        zb = zero_bias if zero_bias is not None else x.new_zeros((w.shape[0],))
        return torch._addmm_activation(zb, x, w.t())
    return x.mm(w.t())


def weight_grad(g: Tensor, y: Optional[Tensor], x: Tensor, w: Tensor, *, out: Optional[Tensor] = None,
                want_masked: bool = True, g_scales: Optional[Scales] = None, x_scales: Optional[Scales] = None,
                premasked: bool = False):
    """(dW, g_pre, Scales of g_pre) of y = relu(x w^T) (y given) or y = x w^T (y None).  dW = g_pre^T x with
    g_pre = g where y > 0 else 0; `premasked`: g already is g_pre (a data gradient whose epilogue applied this layer's ReLU
    backward).  f16x2 arithmetic on the shapes csrc/wgrad_split.hip tiles: column scales of g_pre and x from `g_scales` /
    `x_scales` or from passes (for an unmasked g with y, ONE pass masks, writes g_pre and takes its maxima); otherwise the
    round-3 kernels (mask fused into the weight-gradient kernel).  Falls back to library GEMMs for shapes no kernel tiles."""
    # operands no kernel takes (a misaligned g; a misaligned x: the per-layer forward sent that first-layer input to the library as well)
    aligned = dense_f32(g) and x.data_ptr() % 16 == 0
    plan = plan_layer(g.shape[0], w.shape[0], w.shape[1], relu=y is not None, operands_aligned=True, need_dgrad=False)
    if plan.wgrad == Route.LIBRARY or not aligned:
        gp = g if (y is None or premasked) else torch.ops.aten.threshold_backward(g, y, 0.0)
        gw = torch.mm(gp.t(), x, out=out) if out is not None else gp.t().mm(x)
        return gw, gp, None
    if premasked:
        y = None
    if plan.wgrad == Route.JOBS:     # small batches: the job-table kernel with one job
        gp = g if y is None else torch.ops.aten.threshold_backward(g, y, 0.0)
        gw = ops.linear_wgrad_jobs([(gp, x)], outs=[out] if out is not None else None)[0]
        return gw, gp, (g_scales if y is None else None)
    if plan.wgrad_f16:      # (batched or not: a call of this function is a launch of the layer's own)
        if y is not None:   # mask + maxima in one pass; the weight-gradient kernel then runs without a mask
            r, c, g = ops.maxima(g, y, rows=want_masked, cols=True, write_masked=True)
            g_scales = Scales(r, c)
        else:
            g_scales = ensure_scales(g, g_scales, False, True)
        x_scales = ensure_scales(x, x_scales, False, True)
        gw, _ = ops.linear_wgrad(g, None, x, out=out, g_col_max=g_scales.cols, x_col_max=x_scales.cols)
        return gw, g, g_scales
    gw, gp = ops.linear_wgrad(g, y, x, want_masked=want_masked, out=out, exact_fp32=_ARITH == _FP32)
    return gw, gp, (g_scales if y is None else None)


def backward(gy: Tensor, y: Optional[Tensor], x: Tensor, w: Tensor, need_x: bool, need_w: bool, sink: Optional[Tensor] = None):
    """(gx, gw) of one layer, y = relu(x w^T) (y given) or x w^T (y None): the per-layer backward both the autograd Functions
    and the registered operators run."""
    gy = gy if gy.is_contiguous() else gy.contiguous()
    g, gw, gs = gy, None, None
    if need_w:
        gw, g, gs = weight_grad(gy, y, x, w, out=sink, want_masked=need_x)
    elif y is not None and need_x:
        g = torch.ops.aten.threshold_backward(gy, y, 0.0)      # gy where y > 0 (what autograd does for relu)
    gx = input_grad(g, w, g_scales=gs) if need_x else None
    return gx, gw
