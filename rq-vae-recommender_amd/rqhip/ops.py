"""Tensor-level wrappers over the C ABI (include/rqhip.h).

Every function takes CUDA(ROCm) fp32 tensors, allocates outputs/scratch with torch (the library never
owns memory), enqueues on torch's current stream and returns without synchronising.  CPU tensors are
rejected loudly: the HIP kernels are the product path, there is no host fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch
from torch import Tensor

from . import _lib
from ._lib import MODE_EVAL, MODE_GUMBEL, MODE_ROTATION, MODE_STE, RqHipError, check  # noqa: F401


def _need_gpu(*tensors: Optional[Tensor]) -> torch.device:
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RqHipError(
                "rqhip ops need ROCm device tensors (got a %s tensor); the HIP kernels are the only "
                "implementation of this path -- there is no CPU fallback." % t.device.type)
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RqHipError(f"tensors on different devices: {dev} vs {t.device}")
    return dev


def _f32c(t: Optional[Tensor], name: str) -> Optional[Tensor]:
    if t is None:
        return None
    if t.dtype != torch.float32:
        raise RqHipError(f"{name} must be float32, got {t.dtype}")
    return t.contiguous()


def _ptr(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_RAW_DEVICE = getattr(torch._C, "_cuda_getDevice", None)


def _stream() -> int:
    """The current stream's handle.  `torch.cuda.current_stream().cuda_stream` builds a Stream object per call (11 us of host time, five
    times per eager small-batch step: tools/eager_host_profile.py); the raw getter behind it returns the same handle in well under 1 us."""
    if _RAW_STREAM is not None and _RAW_DEVICE is not None:
        return _RAW_STREAM(_RAW_DEVICE())
    return torch.cuda.current_stream().cuda_stream


class RqForwardOut(NamedTuple):
    ids: Tensor                  # [L,B] int64
    embs: Optional[Tensor]       # [L,B,D]
    residuals: Optional[Tensor]  # [L,B,D]
    emb_sum: Optional[Tensor]    # [B,D]
    loss: Optional[Tensor]       # [B]
    embs_norm: Optional[Tensor]  # [B,L]
    tie_margin: Optional[Tensor] = None  # [L,B] relative top-2 distance margin of each level's argmin


TIE_TAU = 1e-6  # rows with tie_margin below this are near-ties: another correct fp32 evaluation may pick the other code


_SCAN_FLAGS = {"auto": 0, "fp32": _lib.FWD_SCAN_FP32, "valu": _lib.FWD_SCAN_VALU}


def filter_bound(D: int = 32):
    """(c1, c2) of the filtered scan's too-close-to-call threshold at embedding width D (rqhip_filter_bound_d; host-side, no
    GPU needed): c1 = 2^-12 at D = 32, 2^-11 at D = 64."""
    import ctypes as C
    c1, c2 = C.c_float(0), C.c_float(0)
    _lib.lib().rqhip_filter_bound_d(int(D), C.byref(c1), C.byref(c2))
    return c1.value, c2.value


def filter_scores(x: Tensor, codebook: Tensor) -> Tensor:
    """The approximate scores x.c_k - |c_k|^2/2 the filtered scan ranks by (rqhip_filter_scores; test hook of the error
    bound).  x [B,D], codebook [K,D], D = 32 or 64 -> [B,K] fp32."""
    _need_gpu(x, codebook)
    x, codebook = _f32c(x, "x"), _f32c(codebook, "codebook")
    B, D = x.shape
    K = codebook.shape[0]
    with torch.cuda.device(x.device):
        l = _lib.lib()
        out = torch.empty((B, K), dtype=torch.float32, device=x.device)
        wsb = l.rqhip_rq_forward_workspace_bytes(1, K)
        ws = torch.empty((wsb,), dtype=torch.uint8, device=x.device)
        check(l.rqhip_filter_scores(_ptr(x), B, D, _ptr(codebook), K, _ptr(out), _ptr(ws), wsb, _stream()),
              "rqhip_filter_scores")
    return out


class RqSeamOut(NamedTuple):
    res0: Optional[Tensor]       # [B,D]   the input GEMM's result (h given)
    ids: Optional[Tensor]        # [L,B] int64
    emb_sum: Optional[Tensor]    # [B,D]
    loss: Optional[Tensor]       # [B]
    embs_norm: Optional[Tensor]  # [B,L]
    out: Optional[Tensor]        # [B,H]   the output GEMM's result
    out_row_max: Optional[Tensor]   # [H/32, B] int32
    out_col_max: Optional[Tensor]   # [H] int32 (the caller's zeroed buffer)


SEAM_H = 128


def linear_small_supported(M: int, N: int, Kr: int) -> bool:
    """Does rqhip_linear_small take out [M, N] = a [M, Kr] . B (N, Kr multiples of 32)?  Host-side query."""
    return bool(_lib.lib().rqhip_linear_small_supported(int(M), int(N), int(Kr)))


def linear_small_plan(M: int, N: int, Kr: int):
    """(col_blocks, waves) rqhip_linear_small chooses for a shape: `waves` is the number of partial chains an output is summed from."""
    cb, ks = C.c_int(0), C.c_int(0)
    check(_lib.lib().rqhip_linear_small_plan(int(M), int(N), int(Kr), C.byref(cb), C.byref(ks)), "linear_small_plan")
    return cb.value, ks.value


def linear_small(a: Tensor, w: Tensor, *, w_kn: bool = False, epilogue: int = _lib.EPI_STORE, aux: Optional[Tensor] = None,
                 col_blocks: int = 0, waves: int = 0, out: Optional[Tensor] = None) -> Tensor:
    """epilogue(a . w^T) for w [N, Kr] (the forward of a bias-free nn.Linear) or, with w_kn, epilogue(a . w) for w [Kr, N] (its data
    gradient) -- csrc/mlp_small.hip, exact fp32, for batches below 4096 rows (any M is computed correctly).  epilogue: EPI_STORE /
    EPI_RELU / EPI_MASK (out where aux > 0 else 0: the ReLU backward of the layer below).  reference modules/encoder.py:25-38."""
    _need_gpu(a, w, aux, out)
    a, w = _f32c(a, "a"), _f32c(w, "w")
    M, Kr = a.shape
    N = w.shape[1] if w_kn else w.shape[0]
    if (w.shape[0] if w_kn else w.shape[1]) != Kr:
        raise RqHipError(f"linear_small: a {tuple(a.shape)} and w {tuple(w.shape)} (w_kn={w_kn}) do not share the reduction dimension")
    if aux is not None:
        aux = _f32c(aux, "aux")
        if tuple(aux.shape) != (M, N):
            raise RqHipError(f"linear_small: aux must be [{M}, {N}], got {tuple(aux.shape)}")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)

    def launch():
        check(_lib.lib().rqhip_linear_small(_ptr(a), _ptr(w), 1 if w_kn else 0, _ptr(out), M, N, Kr, int(epilogue), _ptr(aux),
                                            int(col_blocks), int(waves), _stream()), "rqhip_linear_small")
    if _RAW_DEVICE is not None and a.device.index == _RAW_DEVICE():     # (the device context manager costs more host time than the launch)
        launch()
    else:
        with torch.cuda.device(a.device):
            launch()
    return out


def rq_seam_supported(D: int, H: int, L: int, K: int) -> bool:
    """Does rqhip_rq_seam take these shapes (D = 32, H = 128, all levels resident in LDS beside the two weights)?  Host-side query."""
    return bool(_lib.lib().rqhip_rq_seam_supported(int(D), int(H), int(L), int(K)))


def rq_seam(*, h: Optional[Tensor] = None, w_in: Optional[Tensor] = None, w_in_transposed: bool = False, h_mask: Optional[Tensor] = None,
            res0: Optional[Tensor] = None, want_res0: bool = True,
            codebooks: Optional[Tensor] = None, mode: int = MODE_EVAL, beta: float = 0.25, want_emb_sum: bool = True,
            want_loss: bool = True, want_norm: bool = True,
            w_out: Optional[Tensor] = None, w_out_transposed: bool = False, epilogue: int = _lib.EPI_STORE,
            out_mask: Optional[Tensor] = None, want_row_max: bool = False, col_max_out: Optional[Tensor] = None) -> RqSeamOut:
    """The RQ <-> MLP seam in one launch (rqhip_rq_seam): [res0 = h' . w_in^T] -> [L quantisation levels] -> [out = epilogue(s . w_out^T)].
    h [B,128] (h' = h where h_mask > 0), w_in [32,128] (or [128,32] with w_in_transposed); without h the rows are `res0` [B,32];
    codebooks [L,K,32] or None (no quantisation: s = the rows); w_out [128,32] (or [32,128] transposed) or None.
    epilogue: EPI_STORE / EPI_RELU / EPI_MASK (out_mask [B,128]).  want_row_max: int32 [4,B] row maxima of `out`; col_max_out: a ZEROED
    int32 [128] that receives its column maxima."""
    _need_gpu(h, w_in, h_mask, res0, codebooks, w_out, out_mask, col_max_out)
    h, w_in, h_mask, res0 = _f32c(h, "h"), _f32c(w_in, "w_in"), _f32c(h_mask, "h_mask"), _f32c(res0, "res0")
    codebooks, w_out, out_mask = _f32c(codebooks, "codebooks"), _f32c(w_out, "w_out"), _f32c(out_mask, "out_mask")
    rows = h if h is not None else res0
    if rows is None or rows.dim() != 2:
        raise RqHipError("rq_seam: h [B,128] or res0 [B,32] must be given")
    B, dev = rows.shape[0], rows.device
    D, H = 32, SEAM_H
    L, K = (codebooks.shape[0], codebooks.shape[1]) if codebooks is not None else (0, 0)
    if h is not None and (tuple(h.shape) != (B, H) or w_in is None or tuple(w_in.shape) != ((H, D) if w_in_transposed else (D, H))
                          or (h_mask is not None and h_mask.shape != h.shape)):
        raise RqHipError(f"rq_seam: h {tuple(h.shape)} / w_in {None if w_in is None else tuple(w_in.shape)} / h_mask do not fit")
    if h is None and tuple(res0.shape) != (B, D):
        raise RqHipError(f"rq_seam: res0 must be [B,{D}]")
    if codebooks is not None and (codebooks.dim() != 3 or codebooks.shape[2] != D):
        raise RqHipError(f"rq_seam: codebooks must be [L,K,{D}]")
    if w_out is not None and tuple(w_out.shape) != ((D, H) if w_out_transposed else (H, D)):
        raise RqHipError(f"rq_seam: w_out {tuple(w_out.shape)} does not fit")
    if epilogue == _lib.EPI_MASK and (out_mask is None or tuple(out_mask.shape) != (B, H)):
        raise RqHipError("rq_seam: EPI_MASK needs out_mask [B,128]")
    if col_max_out is not None and (col_max_out.dtype != torch.int32 or col_max_out.numel() != H or not col_max_out.is_contiguous()):
        raise RqHipError("rq_seam: col_max_out must be a contiguous int32 [128] tensor (zeroed by the caller)")
    with torch.cuda.device(dev):
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
        a = _lib.SeamArgs()
        a.B, a.D, a.H = B, D, H
        a.h, a.h_mask, a.w_in, a.w_in_transposed = _ptr(h), _ptr(h_mask), _ptr(w_in), int(bool(w_in_transposed))
        r0 = f(B, D) if (h is not None and want_res0) else None
        a.res0, a.res0_out = _ptr(res0) if h is None else None, _ptr(r0)
        ids = torch.empty((L, B), dtype=torch.int64, device=dev) if L > 0 else None
        es = f(B, D) if (L > 0 and want_emb_sum) else None
        loss = f(B) if (L > 0 and want_loss) else None
        norms = f(B, L) if (L > 0 and want_norm) else None
        a.codebooks, a.L, a.K, a.mode, a.beta = _ptr(codebooks), L, K, int(mode), float(beta)
        a.ids, a.emb_sum, a.loss, a.embs_norm = _ptr(ids), _ptr(es), _ptr(loss), _ptr(norms)
        out = f(B, H) if w_out is not None else None
        rmx = torch.empty((H // 32, B), dtype=torch.int32, device=dev) if (w_out is not None and want_row_max) else None
        a.w_out, a.w_out_transposed, a.out_epilogue = _ptr(w_out), int(bool(w_out_transposed)), int(epilogue)
        a.out_mask, a.out, a.out_row_max, a.out_col_max = _ptr(out_mask), _ptr(out), _ptr(rmx), _ptr(col_max_out if w_out is not None else None)
        check(_lib.lib().rqhip_rq_seam(C.byref(a), _stream()), "rqhip_rq_seam")
    return RqSeamOut(r0, ids, es, loss, norms, out, rmx, col_max_out if w_out is not None else None)


def rq_forward(res0: Tensor, codebooks: Tensor, mode: int, beta: float, *, want_embs: bool = True,
               want_residuals: bool = True, want_emb_sum: bool = True, want_loss: bool = True,
               want_norm: bool = True, want_margin: bool = False, scan: str = "auto",
               coop_tail: bool = True) -> RqForwardOut:
    """L fused quantisation levels (rqhip_rq_forward_ex).  res0 [B,D], codebooks [L,K,D].
    scan: "auto" (the filtered bf16-split scan where it applies, else fp32 MFMA), "fp32" (always the fp32 MFMA scan),
    "valu" (LDS/VALU scan, D = 32 only) -- same bits from all three, for A/B timing and tests."""
    _need_gpu(res0, codebooks)
    res0, codebooks = _f32c(res0, "res0"), _f32c(codebooks, "codebooks")
    if res0.dim() != 2 or codebooks.dim() != 3 or codebooks.shape[2] != res0.shape[1]:
        raise RqHipError(f"shape mismatch: res0 {tuple(res0.shape)}, codebooks {tuple(codebooks.shape)}")
    B, D = res0.shape
    L, K, _ = codebooks.shape
    dev = res0.device
    with torch.cuda.device(dev):
        l = _lib.lib()
        ids = torch.empty((L, B), dtype=torch.int64, device=dev)
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)  # noqa: E731
        embs = f(L, B, D) if want_embs else None
        residuals = f(L, B, D) if want_residuals else None
        emb_sum = f(B, D) if want_emb_sum else None
        loss = f(B) if want_loss else None
        norm = f(B, L) if want_norm else None
        margin = f(L, B) if want_margin else None
        wsb = l.rqhip_rq_forward_workspace_bytes(L, K)
        ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
        flags = _SCAN_FLAGS[scan] | (0 if coop_tail else _lib.FWD_NO_COOP_TAIL)
        rc = l.rqhip_rq_forward_ex(_ptr(res0), B, D, _ptr(codebooks), L, K, mode, beta, _ptr(ids), _ptr(embs),
                                   _ptr(residuals), _ptr(emb_sum), _ptr(loss), _ptr(norm), _ptr(margin), _ptr(ws), wsb,
                                   flags, _stream())
        check(rc, "rqhip_rq_forward_ex")
    return RqForwardOut(ids, embs, residuals, emb_sum, loss, norm, margin)


_CBGRAD = "ordered"


def use_cbgrad(form: str) -> str:
    """How the TRAINING path (rqhip/autograd.py, rqhip/torch_ops.py) accumulates the codebook gradient where both forms exist (D = 32, STE,
    3 x <= 256 or 3-4 x 1024 codes): "ordered" (default: row order, bit-exact against oracle/rq_oracle.c:rqo_rq_backward_ordered) or
    "matrix" (round 5's experiment, kept selectable: a one-hot matrix product on the bf16 matrix cores, three exact pieces per value, the
    sum's order is the matrix pipe's -- correct to the ordered kernel's own error level and MEASURED SLOWER: 38 vs 32 us at 100 000 rows,
    242 vs 184 us at 1 M, profiles/r05_cbgrad_matrix_ab.txt).  g_res0 has the same bits either way.  Returns the previous setting."""
    global _CBGRAD
    if form not in ("matrix", "ordered"):
        raise ValueError(form)
    before, _CBGRAD = _CBGRAD, form
    return before


def cbgrad_default() -> str:
    return _CBGRAD


def rq_backward(res0: Tensor, codebooks: Tensor, mode: int, beta: float, ids: Tensor, *,
                g_embs: Optional[Tensor] = None, g_embsum: Optional[Tensor] = None,
                g_resid: Optional[Tensor] = None, g_loss: Optional[Tensor] = None,
                need_res0: bool = True, need_codebooks: bool = True, out_g_codebooks: Optional[Tensor] = None,
                cbgrad: str = "ordered"):
    """Closed-form backward of rq_forward (rqhip_rq_backward_ex) -> (g_res0 [B,D] | None, g_codebooks [L,K,D] | None).
    cbgrad: "ordered" (this function's default: the form the oracle restates bit for bit) or "matrix" (see `use_cbgrad`)."""
    _need_gpu(res0, codebooks, ids, g_embs, g_embsum, g_resid, g_loss)
    res0, codebooks = _f32c(res0, "res0"), _f32c(codebooks, "codebooks")
    g_embs, g_embsum = _f32c(g_embs, "g_embs"), _f32c(g_embsum, "g_embsum")
    g_resid, g_loss = _f32c(g_resid, "g_resid"), _f32c(g_loss, "g_loss")
    if ids.dtype != torch.int64:
        raise RqHipError("ids must be int64")
    ids = ids.contiguous()
    B, D = res0.shape
    L, K, _ = codebooks.shape
    if tuple(ids.shape) != (L, B):
        raise RqHipError(f"ids must be [L,B]=({L},{B}), got {tuple(ids.shape)}")
    dev = res0.device
    with torch.cuda.device(dev):
        l = _lib.lib()
        g_res0 = torch.empty((B, D), dtype=torch.float32, device=dev) if need_res0 else None
        g_cb = None
        if need_codebooks:
            g_cb = out_g_codebooks if out_g_codebooks is not None else torch.empty((L, K, D), dtype=torch.float32, device=dev)
            if tuple(g_cb.shape) != (L, K, D) or g_cb.dtype != torch.float32 or not g_cb.is_contiguous():
                raise RqHipError("rq_backward: out_g_codebooks must be a contiguous float32 [L,K,D] tensor")
        wsb = l.rqhip_rq_backward_workspace_bytes(B, D, L, K)
        ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
        rc = l.rqhip_rq_backward_ex(_ptr(res0), B, D, _ptr(codebooks), L, K, mode, beta, _ptr(ids), _ptr(g_embs),
                                    _ptr(g_embsum), _ptr(g_resid), _ptr(g_loss), _ptr(g_res0), _ptr(g_cb), _ptr(ws),
                                    wsb, _lib.BWD_CBGRAD_MATRIX if cbgrad == "matrix" else 0, _stream())
        check(rc, "rqhip_rq_backward_ex")
    return g_res0, g_cb


def kmeans_assign(x: Tensor, centroids: Tensor) -> Tensor:
    """assign[i] = argmin_k |x_i - c_k|^2 (rqhip_kmeans_assign; reference init/kmeans.py:40-43)."""
    _need_gpu(x, centroids)
    x, centroids = _f32c(x, "x"), _f32c(centroids, "centroids")
    B, D = x.shape
    K = centroids.shape[0]
    with torch.cuda.device(x.device):
        assign = torch.empty((B,), dtype=torch.int64, device=x.device)
        rc = _lib.lib().rqhip_kmeans_assign(_ptr(x), B, D, _ptr(centroids), K, _ptr(assign), _stream())
        check(rc, "rqhip_kmeans_assign")
    return assign


def kmeans_update(x: Tensor, assign: Tensor, centroids: Tensor):
    """In-place centroid update (rqhip_kmeans_update; init/kmeans.py:44-59).  `centroids` must be a contiguous
    fp32 device tensor.  Returns (counts [K] int64, shift_sq_max [] fp32), both on the device."""
    _need_gpu(x, assign, centroids)
    x = _f32c(x, "x")
    if centroids.dtype != torch.float32 or not centroids.is_contiguous():
        raise RqHipError("centroids must be contiguous float32 (updated in place)")
    if assign.dtype != torch.int64:
        raise RqHipError("assign must be int64")
    assign = assign.contiguous()
    B, D = x.shape
    K = centroids.shape[0]
    with torch.cuda.device(x.device):
        counts = torch.empty((K,), dtype=torch.int64, device=x.device)
        shift = torch.empty((), dtype=torch.float32, device=x.device)
        rc = _lib.lib().rqhip_kmeans_update(_ptr(x), B, D, _ptr(assign), K, _ptr(centroids), _ptr(counts),
                                            _ptr(shift), _stream())
        check(rc, "rqhip_kmeans_update")
    return counts, shift


def kmeans_lloyd(x: Tensor, centroids: Tensor, assign: Tensor, counts: Tensor, state: Tensor, n_iters: int,
                 stop_threshold: float) -> None:
    """Enqueue a batch of up to n_iters Lloyd iterations (rqhip_kmeans_lloyd); nothing is synchronised.  centroids
    [K,D] fp32 (updated in place), assign [B] int64, counts [K] int64, state [4] int32 -- all device tensors the
    caller keeps across batches (see include/rqhip.h for the state words)."""
    _need_gpu(x, centroids, assign, counts, state)
    if x.dtype != torch.float32 or not x.is_contiguous() or centroids.dtype != torch.float32 or not centroids.is_contiguous():
        raise RqHipError("kmeans_lloyd: x and centroids must be contiguous float32")
    if assign.dtype != torch.int64 or counts.dtype != torch.int64 or state.dtype != torch.int32 or state.numel() < 4:
        raise RqHipError("kmeans_lloyd: assign/counts must be int64, state int32[4]")
    B, D = x.shape
    K = centroids.shape[0]
    with torch.cuda.device(x.device):
        rc = _lib.lib().rqhip_kmeans_lloyd(_ptr(x), B, D, _ptr(centroids), K, _ptr(assign), _ptr(counts), _ptr(state),
                                           int(n_iters), float(stop_threshold), _stream())
        check(rc, "rqhip_kmeans_lloyd")


def kmeans_partial_sums(x: Tensor, centroids: Tensor, assign: Tensor, sums: Tensor, state: Tensor) -> None:
    """Row-sharded Lloyd step, first half (rqhip_kmeans_partial_sums): assign this rank's rows and write their
    per-cluster sums and counts to sums [K, D+1]; the caller all-reduces `sums`."""
    _need_gpu(x, centroids, assign, sums, state)
    B, D = x.shape
    K = centroids.shape[0]
    with torch.cuda.device(centroids.device):
        rc = _lib.lib().rqhip_kmeans_partial_sums(_ptr(x), B, D, _ptr(centroids), K, _ptr(assign), _ptr(sums),
                                                  _ptr(state), _stream())
        check(rc, "rqhip_kmeans_partial_sums")


def kmeans_apply_sums(sums: Tensor, centroids: Tensor, counts: Tensor, state: Tensor, stop_threshold: float) -> None:
    """Row-sharded Lloyd step, second half (rqhip_kmeans_apply_sums): means / shift / flags from the reduced sums."""
    _need_gpu(sums, centroids, counts, state)
    K, D = centroids.shape
    with torch.cuda.device(centroids.device):
        rc = _lib.lib().rqhip_kmeans_apply_sums(_ptr(sums), K, D, _ptr(centroids), _ptr(counts), _ptr(state),
                                                float(stop_threshold), _stream())
        check(rc, "rqhip_kmeans_apply_sums")


def dedup_rank(ids: Tensor, codebook_size: int = 0, *, want_rank: bool = True):
    """Duplicate statistics of semantic-id tuples (rqhip_dedup_rank).  ids [L,B] int64 ->
    (rank [B] int64 | None, n_distinct [] int64): rank[i] = number of earlier rows with row i's tuple
    (reference modules/tokenizer/semids.py:92-108); n_distinct / B = p_unique_ids (modules/rqvae.py:159-167)."""
    _need_gpu(ids)
    if ids.dtype != torch.int64 or ids.dim() != 2:
        raise RqHipError("ids must be an int64 [L,B] tensor")
    ids = ids.contiguous()
    L, B = ids.shape
    dev = ids.device
    with torch.cuda.device(dev):
        l = _lib.lib()
        rank = torch.empty((B,), dtype=torch.int64, device=dev) if want_rank else None
        n = torch.empty((), dtype=torch.int64, device=dev)
        wsb = l.rqhip_dedup_workspace_bytes(B)
        ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
        rc = l.rqhip_dedup_rank(_ptr(ids), B, L, int(codebook_size), _ptr(rank), _ptr(n), _ptr(ws), wsb, _stream())
        check(rc, "rqhip_dedup_rank")
    return rank, n


_DEDUP_WS = {}      # (device index, B) -> workspace: one allocation per batch size instead of one per step


def unique_fraction(ids: Tensor) -> Tensor:
    """p_unique_ids of reference modules/rqvae.py:159-167 for ids [L,B] int64 (B >= 1): the fraction of rows without a later duplicate,
    a device fp32 scalar with torch's `int64 tensor / int` rounding -- one fill + one kernel (rqhip_unique_fraction)."""
    _need_gpu(ids)
    if ids.dtype != torch.int64 or ids.dim() != 2 or ids.shape[1] < 1:
        raise RqHipError("ids must be an int64 [L,B] tensor with B >= 1")
    ids = ids.contiguous()
    L, B = ids.shape
    dev = ids.device
    with torch.cuda.device(dev):
        l = _lib.lib()
        out = torch.empty((), dtype=torch.float32, device=dev)
        key = (dev.index, B)
        ws = _DEDUP_WS.get(key)
        if ws is None or torch.cuda.is_current_stream_capturing():
            ws = torch.empty((l.rqhip_dedup_workspace_bytes(B),), dtype=torch.uint8, device=dev)
            if not torch.cuda.is_current_stream_capturing() and len(_DEDUP_WS) < 16:
                _DEDUP_WS[key] = ws        # (stream-ordered reuse: every use starts with the fill that clears it)
        check(l.rqhip_unique_fraction(_ptr(ids), B, L, _ptr(out), _ptr(ws), ws.numel(), _stream()), "rqhip_unique_fraction")
    return out


def _i64_rows(t: Tensor, name: str) -> Tensor:
    """int64 [rows, cols] with unit column stride (a column slice of a wider table is taken as is)."""
    if t.dtype != torch.int64 or t.dim() != 2:
        raise RqHipError(f"{name} must be an int64 2-D tensor, got {t.dtype} {tuple(t.shape)}")
    cols = t.shape[1]
    if cols > 0 and (t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < cols)):
        t = t.contiguous()
    return t


def _row_stride(t: Tensor) -> int:
    return int(t.stride(0)) if t.shape[0] > 1 else max(int(t.shape[1]), 1)


def prefix_index_build(corpus: Tensor) -> Tensor:
    """Set of all prefixes of the corpus' semantic-id rows (rqhip_prefix_index_build).  corpus [N,H] int64
    (row-strided views are fine) -> opaque uint8 index tensor; keep `corpus` alive and unchanged next to it."""
    _need_gpu(corpus)
    corpus = _i64_rows(corpus, "corpus")
    N, H = corpus.shape
    dev = corpus.device
    with torch.cuda.device(dev):
        l = _lib.lib()
        nbytes = l.rqhip_prefix_index_bytes(N, H)
        if nbytes == 0:
            raise RqHipError(f"prefix_index_build: unsupported corpus shape {tuple(corpus.shape)}")
        index = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        rc = l.rqhip_prefix_index_build(_ptr(corpus), N, H, _row_stride(corpus), _ptr(index), nbytes, _stream())
        check(rc, "rqhip_prefix_index_build")
    return index


def prefix_lookup(index: Tensor, corpus: Tensor, prefix: Tensor) -> Tensor:
    """valid[q] = prefix[q] occurs as the first h ids of some corpus row (rqhip_prefix_lookup); reference
    modules/model.py:169-182.  prefix [P,h] int64 -> bool [P]."""
    _need_gpu(index, corpus, prefix)
    corpus = _i64_rows(corpus, "corpus")
    prefix = _i64_rows(prefix, "prefix")
    N, H = corpus.shape
    P, h = prefix.shape
    dev = corpus.device
    with torch.cuda.device(dev):
        valid = torch.empty((P,), dtype=torch.bool, device=dev)
        rc = _lib.lib().rqhip_prefix_lookup(_ptr(index), index.numel(), _ptr(corpus), N, H, _row_stride(corpus),
                                            _ptr(prefix), P, h, _row_stride(prefix), _ptr(valid), _stream())
        check(rc, "rqhip_prefix_lookup")
    return valid


def topk_first_match(actual: Tensor, top_k: Tensor) -> Tensor:
    """rank[b] = first k with top_k[b,k,:] == actual[b,:], else -1 (rqhip_topk_first_match); the array step of
    the reference's TopKAccumulator.accumulate (evaluate/metrics.py:16-25).  actual [B,D], top_k [B,K,D] int64."""
    _need_gpu(actual, top_k)
    if actual.dtype != torch.int64 or top_k.dtype != torch.int64 or actual.dim() != 2 or top_k.dim() != 3:
        raise RqHipError("topk_first_match: actual [B,D] and top_k [B,K,D] must be int64")
    B, D = actual.shape
    if top_k.shape[0] != B or top_k.shape[2] != D:
        raise RqHipError(f"topk_first_match: top_k {tuple(top_k.shape)} does not match actual {tuple(actual.shape)}")
    K = top_k.shape[1]
    actual, top_k = actual.contiguous(), top_k.contiguous()
    dev = actual.device
    with torch.cuda.device(dev):
        rank = torch.empty((B,), dtype=torch.int64, device=dev)
        rc = _lib.lib().rqhip_topk_first_match(_ptr(actual), _ptr(top_k), B, K, D, _ptr(rank), _stream())
        check(rc, "rqhip_topk_first_match")
    return rank


def sid_item_index_build(corpus: Tensor, rank: Tensor) -> Tensor:
    """Exact map (L-tuple, dedup rank) -> item number of the corpus (rqhip_sid_item_index_build).  corpus [N,L] int64
    (row-strided views are fine), rank [N] int64 = the dedup column (dedup_rank) -> opaque uint8 index tensor; keep
    `corpus` alive and unchanged next to it."""
    _need_gpu(corpus, rank)
    corpus = _i64_rows(corpus, "corpus")
    N, L = corpus.shape
    if rank.dtype != torch.int64 or rank.dim() != 1 or rank.shape[0] != N:
        raise RqHipError(f"sid_item_index_build: rank must be an int64 [{N}] tensor, got {rank.dtype} {tuple(rank.shape)}")
    rank = rank.contiguous()
    dev = corpus.device
    with torch.cuda.device(dev):
        l = _lib.lib()
        nbytes = l.rqhip_sid_item_index_bytes(N)
        index = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        rc = l.rqhip_sid_item_index_build(_ptr(corpus), N, L, _row_stride(corpus), _ptr(rank), _ptr(index), nbytes,
                                          _stream())
        check(rc, "rqhip_sid_item_index_build")
    return index


def sid_item_lookup(index: Tensor, corpus: Tensor, ids: Tensor) -> Tensor:
    """items[p] = the corpus row with tuple ids[p, :L] and dedup rank ids[p, L], else -1 (rqhip_sid_item_lookup).
    ids [P, L+1] int64 (row-strided views are fine) -> int64 [P]."""
    _need_gpu(index, corpus, ids)
    corpus = _i64_rows(corpus, "corpus")
    ids = _i64_rows(ids, "ids")
    N, L = corpus.shape
    P = ids.shape[0]
    if ids.shape[1] != L + 1:
        raise RqHipError(f"sid_item_lookup: ids {tuple(ids.shape)} must have the corpus' {L} ids and the dedup rank per row")
    dev = corpus.device
    with torch.cuda.device(dev):
        items = torch.empty((P,), dtype=torch.int64, device=dev)
        rc = _lib.lib().rqhip_sid_item_lookup(_ptr(index), index.numel(), _ptr(corpus), N, L, _row_stride(corpus),
                                              _ptr(ids), P, _row_stride(ids), _ptr(items), _stream())
        check(rc, "rqhip_sid_item_lookup")
    return items


def sid_items_topn(index: Tensor, corpus: Tensor, beams: Tensor, scores: Tensor, n: int,
                   history: Optional[Tensor] = None):
    """The beams of `generate` expanded to corpus items in ONE launch (rqhip_sid_items_topn; the semantics are in
    include/rqhip.h).  beams [B,k,L] int64 and scores [B,k] fp32, best first; history None or [B, T*(L+1)] int64 in the
    form of batch.sem_ids (row-strided views are fine; an item with a negative id is padding) -> items [B,n] int64
    (-1 padded) and item_scores [B,n] fp32 (-inf padded).  Shapes decide every allocation; nothing is read back."""
    _need_gpu(index, corpus, beams, scores, history)
    corpus = _i64_rows(corpus, "corpus")
    N, L = corpus.shape
    if beams.dtype != torch.int64 or beams.dim() != 3 or beams.shape[2] != L:
        raise RqHipError(f"sid_items_topn: beams must be an int64 [B, k, {L}] tensor, got {beams.dtype} {tuple(beams.shape)}")
    B, k = beams.shape[0], beams.shape[1]
    if scores.dtype != torch.float32 or tuple(scores.shape) != (B, k):
        raise RqHipError(f"sid_items_topn: scores must be a float32 [{B}, {k}] tensor, got {scores.dtype} "
                         f"{tuple(scores.shape)}")
    T = 0
    if history is not None:
        history = _i64_rows(history, "history")
        if history.shape[0] != B or history.shape[1] % (L + 1) != 0:
            raise RqHipError(f"sid_items_topn: history {tuple(history.shape)} must be [{B}, T * {L + 1}]: {L} ids and the "
                             "dedup rank per item")
        T = history.shape[1] // (L + 1)
    n = int(n)
    if not 1 <= n <= 256:
        raise RqHipError(f"sid_items_topn: n={n} items per user (1 <= n <= 256)")
    beams, scores = beams.contiguous(), scores.contiguous()
    dev = corpus.device
    with torch.cuda.device(dev):
        items =torch.empty((B, n), dtype=torch.int64, device=dev)
        item_scores = torch.empty((B, n), dtype=torch.float32, device=dev)
        rc = _lib.lib().rqhip_sid_items_topn(_ptr(index), index.numel(), _ptr(corpus), N, L, _row_stride(corpus),
                                             _ptr(beams), _ptr(scores), B, k, _ptr(history), T,
                                             0 if history is None else _row_stride(history), int(n), _ptr(items),
                                             _ptr(item_scores), _stream())
        check(rc, "rqhip_sid_items_topn")
    return items, item_scores


def beam_step(logits: Tensor, noise: Tensor, parent_scores: Optional[Tensor], parent_ids: Optional[Tensor],
              index: Tensor, corpus: Tensor, n_cands: int, k: int):
    """One hierarchy step of the retrieval model's beam search in one launch (rqhip_beam_step).

    logits [B * beams_in, K] fp32 (unit column stride), noise [B * beams_in, K] Exp(1) draws, parent_scores [B, beams_in]
    fp32 and parent_ids [B, beams_in, h] int64, both None at the first step (beams_in = 1); index / corpus as from
    prefix_index_build.  Returns ids [B, k, h+1] int64, scores [B, k] fp32 and parent [B, k] int64 (the global row
    b * beams_in + beam each kept candidate came from).  Shapes decide every allocation; nothing is read back."""
    _need_gpu(logits, noise, parent_scores, parent_ids, index, corpus)
    if logits.dtype != torch.float32 or logits.dim() != 2:
        raise RqHipError(f"beam_step: logits must be a float32 [rows, K] tensor, got {logits.dtype} {tuple(logits.shape)}")
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    rows, K = logits.shape
    noise = _f32c(noise, "noise")
    if tuple(noise.shape) != (rows, K):
        raise RqHipError(f"beam_step: noise must be [{rows}, {K}], got {tuple(noise.shape)}")
    if parent_ids is None:
        if parent_scores is not None:
            raise RqHipError("beam_step: parent_scores without parent_ids")
        h, beams_in = 0, 1
    else:
        if parent_ids.dtype != torch.int64 or parent_ids.dim() != 3 or parent_scores is None:
            raise RqHipError("beam_step: parent_ids must be int64 [B, beams_in, h] and come with parent_scores")
        beams_in, h = parent_ids.shape[1], parent_ids.shape[2]
        parent_ids = parent_ids.contiguous()
        parent_scores = _f32c(parent_scores, "parent_scores")
    if rows % beams_in != 0:
        raise RqHipError(f"beam_step: {rows} logit rows are not B * beams_in with beams_in = {beams_in}")
    B = rows // beams_in
    if parent_ids is not None and (parent_ids.shape[0] != B or tuple(parent_scores.shape) != (B, beams_in)):
        raise RqHipError(f"beam_step: parent_ids {tuple(parent_ids.shape)} / parent_scores {tuple(parent_scores.shape)} "
                         f"do not match B = {B}, beams_in = {beams_in}")
    corpus = _i64_rows(corpus, "corpus")
    N, H = corpus.shape
    dev = logits.device
    with torch.cuda.device(dev):
        ids = torch.empty((B, k, h + 1), dtype=torch.int64, device=dev)
        scores = torch.empty((B, k), dtype=torch.float32, device=dev)
        parent = torch.empty((B, k), dtype=torch.int64, device=dev)
        l = _lib.lib()
        rc = l.rqhip_beam_step(_ptr(logits), int(logits.stride(0)) if rows > 1 else K, _ptr(noise), _ptr(parent_scores),
                               _ptr(parent_ids), h, B, beams_in, K, int(n_cands), int(k), _ptr(index), index.numel(),
                               _ptr(corpus), N, H, _row_stride(corpus), _ptr(ids), _ptr(scores), _ptr(parent), None, 0,
                               _stream())
        check(rc, "rqhip_beam_step")
    return ids, scores, parent


def beam_topk_step(logits: Tensor, parent_scores: Optional[Tensor], parent_ids: Optional[Tensor], index: Tensor,
                   corpus: Tensor, k: int):
    """One hierarchy step of the exact constrained beam search in one launch (rqhip_beam_topk_step): every code of every
    row is scored by its log-softmax value plus the parent's score, codes whose prefix is not in the corpus score -inf,
    and each user keeps the k best, equal scores (-inf included) to the lower candidate beam * K + code.  No noise.

    logits [B * beams_in, K] fp32 (unit column stride; a row stride is passed through as it is), parent_scores
    [B, beams_in] fp32 and parent_ids [B, beams_in, h] int64, both None at the first step (beams_in = 1); index / corpus
    as from prefix_index_build.  Returns ids [B, k, h+1] int64, scores [B, k] fp32 and parent [B, k] int64 (the global
    row b * beams_in + beam each kept candidate came from).  Shapes decide every allocation; nothing is read back."""
    _need_gpu(logits, parent_scores, parent_ids, index, corpus)
    if logits.dtype != torch.float32 or logits.dim() != 2:
        raise RqHipError(f"beam_topk_step: logits must be a float32 [rows, K] tensor, got {logits.dtype} "
                         f"{tuple(logits.shape)}")
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    rows, K = logits.shape
    if parent_ids is None:
        if parent_scores is not None:
            raise RqHipError("beam_topk_step: parent_scores without parent_ids")
        h, beams_in = 0, 1
    else:
        if parent_ids.dtype != torch.int64 or parent_ids.dim() != 3 or parent_scores is None:
            raise RqHipError("beam_topk_step: parent_ids must be int64 [B, beams_in, h] and come with parent_scores")
        beams_in, h = parent_ids.shape[1], parent_ids.shape[2]
        parent_ids = parent_ids.contiguous()
        parent_scores = _f32c(parent_scores, "parent_scores")
    if beams_in < 1 or rows % beams_in != 0:
        raise RqHipError(f"beam_topk_step: {rows} logit rows are not B * beams_in with beams_in = {beams_in}")
    B = rows // beams_in
    if parent_ids is not None and (parent_ids.shape[0] != B or tuple(parent_scores.shape) != (B, beams_in)):
        raise RqHipError(f"beam_topk_step: parent_ids {tuple(parent_ids.shape)} / parent_scores "
                         f"{tuple(parent_scores.shape)} do not match B = {B}, beams_in = {beams_in}")
    corpus = _i64_rows(corpus, "corpus")
    N, H = corpus.shape
    dev = logits.device
    with torch.cuda.device(dev):
        ids = torch.empty((B, k, h + 1), dtype=torch.int64, device=dev)
        scores = torch.empty((B, k), dtype=torch.float32, device=dev)
        parent = torch.empty((B, k), dtype=torch.int64, device=dev)
        rc = _lib.lib().rqhip_beam_topk_step(_ptr(logits), int(logits.stride(0)) if rows > 1 else K, _ptr(parent_scores),
                                             _ptr(parent_ids), h, B, beams_in, K, int(k), _ptr(index), index.numel(),
                                             _ptr(corpus), N, H, _row_stride(corpus), _ptr(ids), _ptr(scores),
                                             _ptr(parent), _stream())
        check(rc, "rqhip_beam_topk_step")
    return ids, scores, parent


def t5_attention_supported(dtype: torch.dtype, d_kv: int, n_heads: int, Tq: int, Tk: int) -> bool:
    """Whether t5_attention implements this shape (rqhip_t5_attention_supported): fp32, d_kv = 64, Tq and Tk <= 256."""
    return dtype == torch.float32 and bool(
        _lib.lib().rqhip_t5_attention_supported(int(d_kv), int(n_heads), int(Tq), int(Tk)))


def _token_rows(t: Tensor, name: str, copy: bool = True) -> Tensor:
    """A float32 [rows, T, inner] tensor whose tokens lie at one row stride (unit column stride) from a 16-byte boundary;
    copies otherwise (also a contiguous view that starts off the boundary, which contiguous() alone hands back), or raises
    when `copy` is False (the K/V slabs: the point of them is that nothing copies them)."""
    if t.dtype != torch.float32 or t.dim() != 3:
        raise RqHipError(f"t5_attention: {name} must be a float32 [rows, T, heads * 64] tensor, got {t.dtype} "
                         f"{tuple(t.shape)}")
    if t.stride(2) != 1 or t.stride(1) % 4 != 0 or t.stride(0) != t.shape[1] * t.stride(1) or t.data_ptr() % 16 != 0:
        if not copy:
            raise RqHipError(f"t5_attention: {name} must be a 16-byte aligned [positions, rows, heads * 64] slab with "
                             f"one row stride (a multiple of 4), got strides {tuple(t.stride())}")
        t = _aligned16(t.contiguous())
    return t


def _dropout_seed(who: str, seed: Optional[Tensor], **ps: float) -> Optional[int]:
    """Checks a call's one or two dropout probabilities (by the caller's names) and their seed -> the seed pointer, or None."""
    named = lambda: ", ".join(f"{name}={p}" for name, p in ps.items())  # only when raised: this runs once per launch
    live = False
    for p in ps.values():
        if not 0.0 <= p < 1.0:
            raise RqHipError(f"{who}: {named()} outside 0 <= p < 1")
        live = live or p > 0
    if live and (seed is None or seed.dtype != torch.int64 or seed.numel() != 1):
        raise RqHipError(f"{who}: dropout ({named()}) needs `seed`, a one-element int64 device tensor")
    return seed.data_ptr() if live else None


def _packed_side(who: str, t: Tensor, name: str, cu: Optional[Tensor], bound: Optional[int], inner: int, copy: bool = True):
    """One side (q or k / v) of an attention call -> (tensor, groups, rows, bound).  With its table `cu` (int32
    [groups + 1], device) the tensor is 2-D [rows, inner] at one row stride and `bound` the padded length; without, it is
    the dense [groups, T, inner] of t5_attention (`copy`: _token_rows')."""
    if cu is None:
        t = _token_rows(t, name, copy)
        if bound is not None and bound != t.shape[1]:
            raise RqHipError(f"{who}: dense {name} has {t.shape[1]} tokens per row, not the bound {bound}")
        if t.shape[2] != inner:
            raise RqHipError(f"{who}: {name} has {t.shape[2]} columns, not n_heads * 64 = {inner}")
        return t, t.shape[0], t.shape[0] * t.shape[1], t.shape[1]
    if cu.dtype != torch.int32 or cu.dim() != 1 or cu.numel() < 1 or not cu.is_contiguous():
        raise RqHipError(f"{who}: the table of {name} must be a contiguous int32 [groups + 1] tensor, got {cu.dtype} "
                         f"{tuple(cu.shape)}")
    if bound is None or bound < 1:
        raise RqHipError(f"{who}: packed {name} needs its padded length (max_q / max_k >= 1)")
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != inner:
        raise RqHipError(f"{who}: packed {name} must be a float32 [rows, n_heads * 64 = {inner}] tensor, got {t.dtype} "
                         f"{tuple(t.shape)}")
    if t.stride(1) != 1 or t.stride(0) % 4 != 0 or t.stride(0) < inner or t.data_ptr() % 16 != 0:
        t = _aligned16(t.contiguous())
    return t, cu.numel() - 1, t.shape[0], int(bound)


def _attention_args(who: str, q: Tensor, k: Tensor, v: Tensor, n_heads: int, bias_by_delta: Optional[Tensor],
                    key_mask: Optional[Tensor], p: float = 0.0, seed: Optional[Tensor] = None, past: int = 0,
                    anc: Optional[Tensor] = None, packed: Optional[tuple] = None):
    """The checks and copies the nine attention calls share -> (q, k, v, table, key mask, R, Rk, Tq, Tk, inner, seed
    pointer, n_q, n_k).  Each side is dense, or packed behind its table: `packed` is a packed call's (cu_q, cu_k, max_q,
    max_k, causal), and such a call takes one K/V per group and neither mask.  With `anc` k and v are the position slabs,
    which are never copied, and the keys are the positions 0 .. past of each row."""
    cu_q = cu_k = max_q = max_k = None
    if packed is not None:
        cu_q, cu_k, max_q, max_k, causal = packed
        if cu_q is None and cu_k is None:
            raise RqHipError(f"{who}: neither cu_q nor cu_k: the dense call is t5_attention")
        if causal or key_mask is not None:
            raise RqHipError(f"{who}: a cumulative table goes with neither causal nor key_mask (every packed key is valid)")
    inner = int(n_heads) * 64
    q, R, n_q, Tq = _packed_side(who, q, "q", cu_q, max_q, inner)
    if packed is not None:
        if k.shape != v.shape:
            raise RqHipError(f"{who}: k {tuple(k.shape)} / v {tuple(v.shape)} differ")
    elif k.shape != v.shape or k.shape[-1] != inner:
        raise RqHipError(f"{who}: k {tuple(k.shape)} / v {tuple(v.shape)} do not match q {tuple(q.shape)}")
    k, Rk, n_k, Tk = _packed_side(who, k, "k", cu_k, max_k, inner, anc is None)
    v = _packed_side(who, v, "v", cu_k, max_k, inner, anc is None)[0]
    if k.stride(-2) != v.stride(-2):
        if anc is not None:
            raise RqHipError(f"{who}: the k and v slabs must share one row stride")
        k, v = k.contiguous(), v.contiguous()
    if packed is not None and Rk != R:
        raise RqHipError(f"{who}: {R} query groups over {Rk} K/V groups: one K/V per group")
    if anc is not None:
        if (anc.dtype != torch.int32 or anc.dim() != 2 or anc.shape[0] != R or anc.shape[1] < past or anc.stride(1) != 1
                or k.shape[0] <= past or k.shape[1] < R):
            raise RqHipError(f"{who}: anc must be an int32 [R, >= past] table with unit column stride, and the "
                             "slabs must hold position `past` and at least R rows")
        Rk, Tk = R, past + 1
    if bias_by_delta is not None:
        bias_by_delta = _f32c(bias_by_delta, "bias_by_delta")
        if bias_by_delta.dim() != 2 or bias_by_delta.shape[1] != n_heads:
            raise RqHipError(f"{who}: bias_by_delta must be [n_delta, {n_heads}], got {tuple(bias_by_delta.shape)}")
    if key_mask is not None:
        if key_mask.dtype not in (torch.bool, torch.uint8) or tuple(key_mask.shape) != (Rk, Tk):
            raise RqHipError(f"{who}: key_mask must be bool / uint8 [{Rk}, {Tk}], got {key_mask.dtype} "
                             f"{tuple(key_mask.shape)}")
        key_mask = key_mask.contiguous()
    return q, k, v, bias_by_delta, key_mask, R, Rk, Tq, Tk, inner, _dropout_seed(who, seed, p=p), n_q, n_k


def _attention_bwd_args(who: str, q: Tensor, out: Tensor, d_out: Tensor, lse: Tensor, lse_shape: tuple,
                        ml: Optional[Tensor] = None, side: Optional[tuple] = None):
    """What a backward checks of the forward's `out` and `lse` (and `ml`, the long form's) and of d_out -> (out, d_out,
    lse, ml).  `side`: a packed call's (cu_q, Tq, inner), out and d_out then being in q's packed-or-dense layout."""
    if side is None:
        out, d_out = _token_rows(out, "out"), _token_rows(d_out, "d_out")
    else:
        out, d_out = _packed_side(who, out, "out", *side)[0], _packed_side(who, d_out, "d_out", *side)[0]
    if out.shape != q.shape or d_out.shape != q.shape:
        raise RqHipError(f"{who}: out {tuple(out.shape)} / d_out {tuple(d_out.shape)} do not match q {tuple(q.shape)}")
    lse = _f32c(lse, "lse")
    if ml is not None:
        ml = _f32c(ml, "ml")
        if tuple(lse.shape) != lse_shape or tuple(ml.shape) != lse_shape + (2,):
            raise RqHipError(f"{who}: lse must be {list(lse_shape)} and ml {list(lse_shape + (2,))}, got "
                             f"{tuple(lse.shape)} and {tuple(ml.shape)}")
    elif tuple(lse.shape) != lse_shape:
        raise RqHipError(f"{who}: lse must be {list(lse_shape)}, got {tuple(lse.shape)}")
    return out, d_out, lse, ml


def _attention_grads(q: Tensor, k: Tensor, bias_by_delta: Optional[Tensor], scratch: Optional[tuple]):
    """A backward's outputs on the current device -> (dq like q, dk and dv like k, dtable like the bias table or None,
    and a float32 buffer of shape `scratch` or None: the short kernels' [R * H, Tq + Tk - 1] partial bias gradients,
    which go with a table, or the long kernels' workspace)."""
    dq = torch.empty(q.shape, dtype=torch.float32, device=q.device)
    dk = torch.empty(k.shape, dtype=torch.float32, device=q.device)
    dv = torch.empty(k.shape, dtype=torch.float32, device=q.device)
    dtable = None if bias_by_delta is None else torch.empty_like(bias_by_delta)
    return dq, dk, dv, dtable, None if scratch is None else torch.empty(scratch, dtype=torch.float32, device=q.device)


def t5_attention(q: Tensor, k: Tensor, v: Tensor, n_heads: int, *, bias_by_delta: Optional[Tensor] = None,
                 bias_offset: int = 0, key_mask: Optional[Tensor] = None, causal: bool = False, past: int = 0,
                 anc: Optional[Tensor] = None) -> Tensor:
    """softmax(q k^T + bias + mask) v for every row and head in one launch (rqhip_t5_attention), T5 semantics, fp32.

    q [R, Tq, n_heads * 64] as the q Linear wrote it; returns [R, Tq, n_heads * 64] as the o Linear reads it.
    Dense K/V: k, v [Rk, Tk, n_heads * 64], R a multiple of Rk (rows b * R / Rk .. read group b).  Cached decode step
    (anc [R, >= past] int32, Tq = 1): k, v are the position slabs [positions, slab_rows, n_heads * 64]; key t < past of
    row r is row anc[r, t] of slab t, key `past` is row r of slab `past`.
    bias_by_delta [n_delta, n_heads]: table[(j - i - past) + bias_offset] is added.  key_mask [Rk, Tk] bool / uint8
    (0 = masked), causal keeps j <= i + past; masked scores get finfo(float32).min added."""
    _need_gpu(q, k, v, bias_by_delta, key_mask, anc)
    q, k, v, bias_by_delta, key_mask, R, Rk, Tq, Tk, inner, _, _, _ = _attention_args(
        "t5_attention", q, k, v, n_heads, bias_by_delta, key_mask, past=past, anc=anc)
    slab_rows, ld_anc = (0, 0) if anc is None else (k.shape[1], int(anc.stride(0)))
    dev = q.device
    with torch.cuda.device(dev):
        out = torch.empty((R, Tq, inner), dtype=torch.float32, device=dev)
        rc = _lib.lib().rqhip_t5_attention(
            _ptr(q), int(q.stride(1)), _ptr(k), _ptr(v), int(k.stride(1)), R, Rk, int(n_heads), 64, Tq, Tk,
            _ptr(bias_by_delta), 0 if bias_by_delta is None else bias_by_delta.shape[0], int(bias_offset),
            _ptr(key_mask), int(bool(causal)), int(past), _ptr(anc), ld_anc, slab_rows, _ptr(out), inner, _stream())
        check(rc, "rqhip_t5_attention")
    return out


def t5_attention_bwd_supported(dtype: torch.dtype, d_kv: int, n_heads: int, Tq: int, Tk: int) -> bool:
    """Whether t5_attention_fwd_train / t5_attention_bwd implement this shape (rqhip_t5_attention_bwd_supported): fp32,
    d_kv = 64, Tq and Tk <= 256."""
    return dtype == torch.float32 and bool(
        _lib.lib().rqhip_t5_attention_bwd_supported(int(d_kv), int(n_heads), int(Tq), int(Tk)))


_M32 = 0xFFFFFFFF


def _fmix32(h: Tensor) -> Tensor:
    """murmur3's 32-bit finaliser on int64 tensors holding values below 2^32 (products wrap; their low 32 bits hold)."""
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & _M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & _M32
    return h ^ (h >> 16)


def t5_attention_dropout_keep(seed, R: int, H: int, Tq: int, Tk: int, p: float) -> Tensor:
    """The kernels' dropout decision as a bool [R, H, Tq, Tk] (True = kept), in torch integer operations on the seed's
    device (`seed`: an int or a one-element int64 tensor, host or device).  Element x = ((r * H + h) * Tq + i) * Tk + j is
    kept iff fmix((fmix(lo(seed) ^ lo(x)) ^ hi(seed) ^ hi(x) * 0x85EBCA6B) + 0x9E3779B9) >= round(p * 2^32)
    (include/rqhip.h)."""
    if not 0.0 <= p < 1.0:
        raise RqHipError(f"t5_attention_dropout_keep: p={p} outside 0 <= p < 1")
    if not isinstance(seed, Tensor):
        seed = torch.tensor(int(seed), dtype=torch.int64)
    seed = seed.reshape(()).to(torch.int64)
    x = torch.arange(R * H * Tq * Tk, dtype=torch.int64, device=seed.device)
    h = _fmix32((seed & _M32) ^ (x & _M32))
    h = _fmix32(((h ^ ((seed >> 32) & _M32) ^ ((((x >> 32) & _M32) * 0x85EBCA6B) & _M32)) + 0x9E3779B9) & _M32)
    return (h >= min(int(round(p * 4294967296.0)), _M32)).view(R, H, Tq, Tk)


def t5_attention_fwd_train(q: Tensor, k: Tensor, v: Tensor, n_heads: int, *, bias_by_delta: Optional[Tensor] = None,
                           bias_offset: int = 0, key_mask: Optional[Tensor] = None, causal: bool = False, p: float = 0.0,
                           seed: Optional[Tensor] = None):
    """t5_attention's dense form for training in one launch (rqhip_t5_attention_fwd_train) -> (out [R, Tq, n_heads * 64],
    lse [R, n_heads, Tq]).  k, v [R, Tk, n_heads * 64]; with p > 0 the normalised weights are dropped by
    t5_attention_dropout_keep(seed, ...) and scaled by 1 / (1 - p); `seed` is a one-element int64 device tensor the host
    never reads.  At p = 0 `out` has the bits of t5_attention."""
    _need_gpu(q, k, v, bias_by_delta, key_mask, seed)
    q, k, v, bias_by_delta, key_mask, R, Rk, Tq, Tk, inner, seed_ptr, _, _ = _attention_args(
        "t5_attention_fwd_train", q, k, v, n_heads, bias_by_delta, key_mask, p, seed)
    dev = q.device
    with torch.cuda.device(dev):
        out = torch.empty((R, Tq, inner), dtype=torch.float32, device=dev)
        lse = torch.empty((R, int(n_heads), Tq), dtype=torch.float32, device=dev)
        rc = _lib.lib().rqhip_t5_attention_fwd_train(
            _ptr(q), int(q.stride(1)), _ptr(k), _ptr(v), int(k.stride(1)), R, Rk, int(n_heads), 64, Tq, Tk,
            _ptr(bias_by_delta), 0 if bias_by_delta is None else bias_by_delta.shape[0], int(bias_offset),
            _ptr(key_mask), int(bool(causal)), float(p), seed_ptr, _ptr(out), inner, _ptr(lse), _stream())
        check(rc, "rqhip_t5_attention_fwd_train")
    return out, lse


def t5_attention_bwd(q: Tensor, k: Tensor, v: Tensor, out: Tensor, lse: Tensor, d_out: Tensor, n_heads: int, *,
                     bias_by_delta: Optional[Tensor] = None, bias_offset: int = 0, key_mask: Optional[Tensor] = None,
                     causal: bool = False, p: float = 0.0, seed: Optional[Tensor] = None):
    """The gradients of t5_attention_fwd_train in one attention launch (rqhip_t5_attention_bwd) -> (dq [R, Tq, inner],
    dk, dv [R, Tk, inner], dtable [n_delta, n_heads] or None without a bias table).  The arguments are the forward's, its
    `out` and `lse`, and d_out [R, Tq, inner]; the weights are recomputed, the dropout decisions too."""
    _need_gpu(q, k, v, out, lse, d_out, bias_by_delta, key_mask, seed)
    q, k, v, bias_by_delta, key_mask, R, Rk, Tq, Tk, inner, seed_ptr, _, _ = _attention_args(
        "t5_attention_bwd", q, k, v, n_heads, bias_by_delta, key_mask, p, seed)
    out, d_out, lse, _ = _attention_bwd_args("t5_attention_bwd", q, out, d_out, lse, (R, int(n_heads), Tq))
    with torch.cuda.device(q.device):
        dq, dk, dv, dtable, partial = _attention_grads(
            q, k, bias_by_delta, None if bias_by_delta is None else (R * int(n_heads), Tq + Tk - 1))
        rc = _lib.lib().rqhip_t5_attention_bwd(
            _ptr(q), int(q.stride(1)), _ptr(k), _ptr(v), int(k.stride(1)), _ptr(out), int(out.stride(1)), _ptr(lse),
            _ptr(d_out), int(d_out.stride(1)), R, Rk, int(n_heads), 64, Tq, Tk, _ptr(bias_by_delta),
            0 if bias_by_delta is None else bias_by_delta.shape[0], int(bias_offset), _ptr(key_mask), int(bool(causal)),
            float(p), seed_ptr, _ptr(dq), _ptr(dk), _ptr(dv), _ptr(dtable), _ptr(partial), _stream())
        check(rc, "rqhip_t5_attention_bwd")
    return dq, dk, dv, dtable


def t5_attention_packed_supported(dtype: torch.dtype, d_kv: int, n_heads: int, Tq: int, Tk: int) -> bool:
    """Whether the packed attention calls implement these padded BOUNDS (rqhip_t5_attention_packed_supported): fp32,
    d_kv = 64, Tq and Tk <= 256."""
    return dtype == torch.float32 and bool(
        _lib.lib().rqhip_t5_attention_packed_supported(int(d_kv), int(n_heads), int(Tq), int(Tk)))


def t5_attention_packed(q: Tensor, k: Tensor, v: Tensor, n_heads: int, *, cu_q: Optional[Tensor] = None,
                        cu_k: Optional[Tensor] = None, max_q: Optional[int] = None, max_k: Optional[int] = None,
                        bias_by_delta: Optional[Tensor] = None, bias_offset: int = 0, key_mask: Optional[Tensor] = None,
                        causal: bool = False) -> Tensor:
    """t5_attention on packed variable-length rows in one launch (rqhip_t5_attention_packed): R groups, one K/V each.
    With cu_k (int32 [R + 1] on the device) k, v are [n_k, n_heads * 64] and group b's keys the rows cu_k[b] ..
    cu_k[b + 1] - 1, at most max_k (the padded length); without, k, v are the dense [R, Tk, n_heads * 64].  cu_q / max_q do
    the same for q and the result.  The bias table is indexed by j - i as in the padded call.  key_mask and causal must
    stay None / False: they are here to be rejected.  On every valid element the result has the bits of t5_attention on
    the scattered tensors with the prefix key mask."""
    _need_gpu(q, k, v, bias_by_delta, key_mask, cu_q, cu_k)
    who = "t5_attention_packed"
    q, k, v, bias_by_delta, _, R, _, Tq, Tk, inner, _, n_q, n_k = _attention_args(
        who, q, k, v, n_heads, bias_by_delta, key_mask, packed=(cu_q, cu_k, max_q, max_k, causal))
    dev = q.device
    with torch.cuda.device(dev):
        out = torch.empty(q.shape, dtype=torch.float32, device=dev)
        rc = _lib.lib().rqhip_t5_attention_packed(
            _ptr(q), int(q.stride(-2)), _ptr(k), _ptr(v), int(k.stride(-2)), R, n_q, n_k, int(n_heads), 64, Tq, Tk,
            _ptr(cu_q), _ptr(cu_k), _ptr(bias_by_delta), 0 if bias_by_delta is None else bias_by_delta.shape[0],
            int(bias_offset), None, 0, _ptr(out), inner, _stream())
        check(rc, "rqhip_t5_attention_packed")
    return out


def t5_attention_packed_beams(q: Tensor, k: Tensor, v: Tensor, n_heads: int, *, cu_k: Tensor, max_k: int,
                              beams: int) -> Tensor:
    """The cross-attention of a cached decode step over packed encoder rows in one launch
    (rqhip_t5_attention_packed_beams), inference only: q [R, Tq, n_heads * 64] dense, R = groups * beams, rows
    b * beams .. b * beams + beams - 1 reading group b, whose keys are rows cu_k[b] .. cu_k[b + 1] - 1 of k, v
    [n_k, n_heads * 64] (cu_k int32 [R // beams + 1] on the device, at most max_k keys a group).  No bias table and no
    mask.  q and k / v may be views with a larger row stride (the grouped projections' and cross_kv's outputs): nothing
    is copied.  With beams = 1 the result has the bits of t5_attention_packed(cu_q=None), and on every query those of
    t5_attention on the scattered k / v with the prefix key mask."""
    _need_gpu(q, k, v, cu_k)
    who = "t5_attention_packed_beams"
    inner, beams = int(n_heads) * 64, int(beams)
    q, R, _, Tq = _packed_side(who, q, "q", None, None, inner)
    if beams < 1 or R % beams != 0:
        raise RqHipError(f"{who}: beams={beams} does not divide the R={R} query rows")
    if cu_k is None:
        raise RqHipError(f"{who}: cu_k is required (the dense call is t5_attention)")
    if k.shape != v.shape:
        raise RqHipError(f"{who}: k {tuple(k.shape)} / v {tuple(v.shape)} differ")
    k, Rk, n_k, Tk = _packed_side(who, k, "k", cu_k, max_k, inner)
    v = _packed_side(who, v, "v", cu_k, max_k, inner)[0]
    if Rk != R // beams:
        raise RqHipError(f"{who}: the table of k must be a contiguous int32 [R // beams + 1 = {R // beams + 1}] tensor, "
                         f"got {tuple(cu_k.shape)}")
    if k.stride(0) != v.stride(0):
        k, v = k.contiguous(), v.contiguous()
    dev = q.device
    with torch.cuda.device(dev):
        out = torch.empty((R, Tq, inner), dtype=torch.float32, device=dev)
        rc = _lib.lib().rqhip_t5_attention_packed_beams(
            _ptr(q), int(q.stride(1)), _ptr(k), _ptr(v), int(k.stride(0)), R, Rk, n_k, int(n_heads), 64, Tq, Tk,
            _ptr(cu_k), _ptr(out), inner, _stream())
        check(rc, "rqhip_t5_attention_packed_beams")
    return out


def t5_attention_packed_fwd_train(q: Tensor, k: Tensor, v: Tensor, n_heads: int, *, cu_q: Optional[Tensor] = None,
                                  cu_k: Optional[Tensor] = None, max_q: Optional[int] = None,
                                  max_k: Optional[int] = None, bias_by_delta: Optional[Tensor] = None,
                                  bias_offset: int = 0, key_mask: Optional[Tensor] = None, causal: bool = False,
                                  p: float = 0.0, seed: Optional[Tensor] = None):
    """t5_attention_packed for training (rqhip_t5_attention_packed_fwd_train) -> (out, lse); lse is [n_q, n_heads] with
    cu_q and [R, n_heads, Tq] without.  The dropout decision of weight (b, h, i, j) is the padded call's,
    t5_attention_dropout_keep(seed, R, H, max_q, max_k, p)[b, h, i, j].  At p = 0 `out` has the bits of
    t5_attention_packed."""
    _need_gpu(q, k, v, bias_by_delta, key_mask, cu_q, cu_k, seed)
    who = "t5_attention_packed_fwd_train"
    q, k, v, bias_by_delta, _, R, _, Tq, Tk, inner, seed_ptr, n_q, n_k = _attention_args(
        who, q, k, v, n_heads, bias_by_delta, key_mask, p, seed, packed=(cu_q, cu_k, max_q, max_k, causal))
    dev = q.device
    with torch.cuda.device(dev):
        out = torch.empty(q.shape, dtype=torch.float32, device=dev)
        lse = torch.empty((n_q, int(n_heads)) if cu_q is not None else (R, int(n_heads), Tq), dtype=torch.float32,
                          device=dev)
        rc = _lib.lib().rqhip_t5_attention_packed_fwd_train(
            _ptr(q), int(q.stride(-2)), _ptr(k), _ptr(v), int(k.stride(-2)), R, n_q, n_k, int(n_heads), 64, Tq, Tk,
            _ptr(cu_q), _ptr(cu_k), _ptr(bias_by_delta), 0 if bias_by_delta is None else bias_by_delta.shape[0],
            int(bias_offset), None, 0, float(p), seed_ptr, _ptr(out), inner, _ptr(lse), _stream())
        check(rc, "rqhip_t5_attention_packed_fwd_train")
    return out, lse


def t5_attention_packed_bwd(q: Tensor, k: Tensor, v: Tensor, out: Tensor, lse: Tensor, d_out: Tensor, n_heads: int, *,
                            cu_q: Optional[Tensor] = None, cu_k: Optional[Tensor] = None, max_q: Optional[int] = None,
                            max_k: Optional[int] = None, bias_by_delta: Optional[Tensor] = None, bias_offset: int = 0,
                            key_mask: Optional[Tensor] = None, causal: bool = False, p: float = 0.0,
                            seed: Optional[Tensor] = None):
    """The gradients of t5_attention_packed_fwd_train in one attention launch (rqhip_t5_attention_packed_bwd) -> (dq in
    q's layout, dk, dv in k's, dtable [n_delta, n_heads] or None).  The arguments are the forward's, its `out` and `lse`,
    and d_out in q's layout."""
    _need_gpu(q, k, v, out, lse, d_out, bias_by_delta, key_mask, cu_q, cu_k, seed)
    who = "t5_attention_packed_bwd"
    q, k, v, bias_by_delta, _, R, _, Tq, Tk, inner, seed_ptr, n_q, n_k = _attention_args(
        who, q, k, v, n_heads, bias_by_delta, key_mask, p, seed, packed=(cu_q, cu_k, max_q, max_k, causal))
    out, d_out, lse, _ = _attention_bwd_args(
        who, q, out, d_out, lse, (n_q, int(n_heads)) if cu_q is not None else (R, int(n_heads), Tq), side=(cu_q, Tq, inner))
    with torch.cuda.device(q.device):
        dq, dk, dv, dtable, partial = _attention_grads(
            q, k, bias_by_delta, None if bias_by_delta is None else (R * int(n_heads), Tq + Tk - 1))
        rc = _lib.lib().rqhip_t5_attention_packed_bwd(
            _ptr(q), int(q.stride(-2)), _ptr(k), _ptr(v), int(k.stride(-2)), _ptr(out), int(out.stride(-2)), _ptr(lse),
            _ptr(d_out), int(d_out.stride(-2)), R, n_q, n_k, int(n_heads), 64, Tq, Tk, _ptr(cu_q), _ptr(cu_k),
            _ptr(bias_by_delta), 0 if bias_by_delta is None else bias_by_delta.shape[0], int(bias_offset), None, 0,
            float(p), seed_ptr, _ptr(dq), _ptr(dk), _ptr(dv), _ptr(dtable), _ptr(partial), _stream())
        check(rc, "rqhip_t5_attention_packed_bwd")
    return dq, dk, dv, dtable


def rows_pack_supported(dtype: torch.dtype, d: int) -> bool:
    """Whether rows_pack / rows_unpack implement this row width (rqhip_rows_pack_supported): fp32, d a multiple of 4."""
    return dtype == torch.float32 and bool(_lib.lib().rqhip_rows_pack_supported(int(d)))


def _rows_table(who: str, cu: Tensor, B: int) -> None:
    if cu.dtype != torch.int32 or cu.dim() != 1 or cu.numel() != B + 1 or not cu.is_contiguous():
        raise RqHipError(f"{who}: cu must be a contiguous int32 [{B + 1}] tensor, got {cu.dtype} {tuple(cu.shape)}")


def rows_pack(x: Tensor, cu: Tensor, N: int) -> Tensor:
    """Padded rows x [B, T, d] -> packed [N, d] in one launch (rqhip_rows_pack): the first cu[b + 1] - cu[b] tokens of
    row b land at rows cu[b] ..; cu is an int32 [B + 1] device table with cu[B] = N, and N is the caller's (host) count.
    Exact copies."""
    _need_gpu(x, cu)
    x = _f32c(x, "x")
    if x.dim() != 3:
        raise RqHipError(f"rows_pack: x must be [B, T, d], got {tuple(x.shape)}")
    B, T, d = x.shape
    _rows_table("rows_pack", cu, B)
    x = _aligned16(x)
    with torch.cuda.device(x.device):
        out = torch.empty((int(N), d), dtype=torch.float32, device=x.device)
        check(_lib.lib().rqhip_rows_pack(_ptr(x), _ptr(cu), B, T, d, int(N), _ptr(out), _stream()), "rqhip_rows_pack")
    return out


def rows_unpack(x: Tensor, cu: Tensor, B: int, T: int) -> Tensor:
    """Packed rows x [N, d] -> padded [B, T, d] in one launch (rqhip_rows_unpack), the padded tail of every row zero:
    the inverse of rows_pack and its backward."""
    _need_gpu(x, cu)
    x = _f32c(x, "x")
    if x.dim() != 2:
        raise RqHipError(f"rows_unpack: x must be [N, d], got {tuple(x.shape)}")
    N, d = x.shape
    _rows_table("rows_unpack", cu, int(B))
    x = _aligned16(x)
    with torch.cuda.device(x.device):
        out = torch.empty((int(B), int(T), d), dtype=torch.float32, device=x.device)
        check(_lib.lib().rqhip_rows_unpack(_ptr(x), _ptr(cu), int(B), int(T), d, N, _ptr(out), _stream()),
              "rqhip_rows_unpack")
    return out


# the arithmetics of t5_ffn_*, t5_proj_* and t5_attention_long* (include/rqhip.h): storage is fp32 in both
T5_ARITHS = ("fp32", "bf16")


def _arith_entry(who: str, arith: str):
    """The C entry point of `who` in the arithmetic `arith`: "fp32" (exact fp32 products) or "bf16" (operands rounded to
    bf16, exact products, fp32 accumulation)."""
    if arith not in T5_ARITHS:
        raise RqHipError(f"{who}: arith must be one of {T5_ARITHS}, got {arith!r}")
    name = f"rqhip_{who}" + ("_bf16" if arith == "bf16" else "")
    return getattr(_lib.lib(), name), name


T5_SAVED = ("fp32", "bf16")   # what t5_ffn_fwd keeps for t5_ffn_bwd: the fp32 h, or blocked bf16 activation images


class T5MatmulForm(NamedTuple):
    """Which form a t5_ffn_* / t5_proj_* call takes: its arithmetic (T5_ARITHS), whether it reads bf16 weight images
    (bf16_images) and whether the feed-forward keeps bf16 saved activations.  The five legal values are the constants
    below; images and saved activations hold bf16 roundings, so only the "bf16" arithmetic has them."""
    arith: str
    images: bool = False
    saved: bool = False

    def keywords(self, w_images=None) -> dict:
        """The keywords that make a t5_ffn_* / t5_proj_* call take this form, reading `w_images` where it has images:
        each keyword only off its default, so T5_FP32 is the plain call."""
        kw = {} if self.arith == "fp32" else {"arith": self.arith}
        if self.images:
            kw["w_images"] = w_images
        if self.saved:
            kw["saved"] = "bf16"
        return kw


T5_FP32 = T5MatmulForm("fp32")
T5_BF16 = T5MatmulForm("bf16")
T5_BF16_IMAGES = T5MatmulForm("bf16", images=True)
T5_BF16_SAVED = T5MatmulForm("bf16", saved=True)
T5_BF16_IMAGES_SAVED = T5MatmulForm("bf16", images=True, saved=True)
_T5_ENTRY_SUFFIX = {T5_FP32: "", T5_BF16: "_bf16", T5_BF16_IMAGES: "_bf16w", T5_BF16_SAVED: "_bf16a",
                    T5_BF16_IMAGES_SAVED: "_bf16wa"}


def t5_matmul_entry(who: str, arith: str = "fp32", w_images=None, saved: str = "fp32"):
    """The keywords of the t5_ffn_* / t5_proj_* call `who` -> (its T5MatmulForm, the C entry point rqhip_<who><suffix>,
    that name).  Complaints, in this order: an unknown `saved`, an unknown arithmetic, w_images off "bf16", saved="bf16"
    off "bf16"."""
    if saved not in T5_SAVED:
        raise RqHipError(f"{who}: saved must be one of {T5_SAVED}, got {saved!r}")
    if arith not in T5_ARITHS:
        raise RqHipError(f"{who}: arith must be one of {T5_ARITHS}, got {arith!r}")
    if w_images is not None and arith != "bf16":
        raise RqHipError(f'{who}: w_images belong to arith="bf16" (the images hold bf16 roundings), got arith={arith!r}')
    if saved == "bf16" and arith != "bf16":
        raise RqHipError(f'{who}: saved="bf16" belongs to arith="bf16" (the images hold its bf16 operands), got arith={arith!r}')
    form = T5MatmulForm(arith, w_images is not None, saved == "bf16")
    name = f"rqhip_{who}{_T5_ENTRY_SUFFIX[form]}"
    return form, getattr(_lib.lib(), name), name


def _image(who: str, img, name: str, shape, dev) -> Tensor:
    """A bf16 weight image as the kernels read it: a dense, 16-byte aligned bfloat16 tensor of `shape` on `dev`."""
    if not isinstance(img, Tensor) or img.dtype != torch.bfloat16 or tuple(img.shape) != tuple(shape) or img.device != dev:
        got = f"{img.dtype} {tuple(img.shape)} on {img.device}" if isinstance(img, Tensor) else repr(type(img))
        raise RqHipError(f"{who}: {name} must be a bfloat16 {list(shape)} image on {dev} (ops.bf16_images), got {got}")
    if not img.is_contiguous() or img.data_ptr() % 16:
        raise RqHipError(f"{who}: {name} must be dense and 16-byte aligned")
    return img


T5_ATTENTION_LONG_CHUNK = 128   # RQHIP_T5_ATTENTION_LONG_CHUNK: keys a workgroup holds in LDS at a time
T5_ATTENTION_LONG_QBLOCK = 64   # RQHIP_T5_ATTENTION_LONG_QBLOCK: query rows of a workgroup


def t5_attention_long_supported(dtype: torch.dtype, d_kv: int, n_heads: int, Tq: int, Tk: int) -> bool:
    """Whether t5_attention_long, t5_attention_long_fwd_train and t5_attention_long_bwd implement this shape
    (rqhip_t5_attention_long_supported): fp32, d_kv = 64, Tq and Tk <= 2048."""
    return dtype == torch.float32 and bool(
        _lib.lib().rqhip_t5_attention_long_supported(int(d_kv), int(n_heads), int(Tq), int(Tk)))


def t5_attention_long(q: Tensor, k: Tensor, v: Tensor, n_heads: int, *, bias_by_delta: Optional[Tensor] = None,
                      bias_offset: int = 0, key_mask: Optional[Tensor] = None, causal: bool = False,
                      arith: str = "fp32") -> Tensor:
    """t5_attention's dense form for up to 2048 tokens in one launch (rqhip_t5_attention_long, csrc/t5_attention_long.hip):
    the keys are walked in chunks of T5_ATTENTION_LONG_CHUNK with an online softmax.  q [R, Tq, n_heads * 64], k, v
    [Rk, Tk, n_heads * 64], R a multiple of Rk; bias_by_delta, bias_offset, key_mask and causal as in t5_attention.  No
    ancestor table and no `past`: the cached decode step stays on t5_attention.  arith: "fp32", or "bf16"
    (rqhip_t5_attention_long_bf16: q, k, v and the unnormalised weights rounded to bf16 as matrix operands, the softmax in
    fp32 on unrounded values; all tensors stay float32)."""
    fn, fn_name = _arith_entry("t5_attention_long", arith)
    _need_gpu(q, k, v, bias_by_delta, key_mask)
    q, k, v, bias_by_delta, key_mask, R, Rk, Tq, Tk, inner, _, _, _ = _attention_args(
        "t5_attention_long", q, k, v, n_heads, bias_by_delta, key_mask)
    dev = q.device
    with torch.cuda.device(dev):
        out = torch.empty((R, Tq, inner), dtype=torch.float32, device=dev)
        rc = fn(_ptr(q), int(q.stride(1)), _ptr(k), _ptr(v), int(k.stride(1)), R, Rk, int(n_heads), 64, Tq, Tk,
                _ptr(bias_by_delta), 0 if bias_by_delta is None else bias_by_delta.shape[0], int(bias_offset),
                _ptr(key_mask), int(bool(causal)), 0, None, _ptr(out), inner, _stream())
        check(rc, fn_name)
    return out


def t5_attention_long_fwd_train(q: Tensor, k: Tensor, v: Tensor, n_heads: int, *, bias_by_delta: Optional[Tensor] = None,
                                bias_offset: int = 0, key_mask: Optional[Tensor] = None, causal: bool = False,
                                p: float = 0.0, seed: Optional[Tensor] = None, arith: str = "fp32"):
    """t5_attention_fwd_train for up to 2048 tokens in one launch (rqhip_t5_attention_long_fwd_train) -> (out
    [R, Tq, n_heads * 64], lse [R, n_heads, Tq], ml [R, n_heads, Tq, 2]: each row's final running max and sum, which the
    backward reads).  The dropout decision is t5_attention_dropout_keep(seed, ...), unchanged.  arith: "fp32" or "bf16",
    as t5_attention_long's (rqhip_t5_attention_long_fwd_train_bf16); lse and ml of a "bf16" forward are read by the
    "bf16" backward only."""
    fn, fn_name = _arith_entry("t5_attention_long_fwd_train", arith)
    _need_gpu(q, k, v, bias_by_delta, key_mask, seed)
    q, k, v, bias_by_delta, key_mask, R, Rk, Tq, Tk, inner, seed_ptr, _, _ = _attention_args(
        "t5_attention_long_fwd_train", q, k, v, n_heads, bias_by_delta, key_mask, p, seed)
    dev = q.device
    with torch.cuda.device(dev):
        out = torch.empty((R, Tq, inner), dtype=torch.float32, device=dev)
        lse = torch.empty((R, int(n_heads), Tq), dtype=torch.float32, device=dev)
        ml = torch.empty((R, int(n_heads), Tq, 2), dtype=torch.float32, device=dev)
        rc = fn(_ptr(q), int(q.stride(1)), _ptr(k), _ptr(v), int(k.stride(1)), R, Rk, int(n_heads), 64, Tq, Tk,
                _ptr(bias_by_delta), 0 if bias_by_delta is None else bias_by_delta.shape[0], int(bias_offset),
                _ptr(key_mask), int(bool(causal)), float(p), seed_ptr, _ptr(out), inner, _ptr(lse), _ptr(ml), _stream())
        check(rc, fn_name)
    return out, lse, ml


def t5_attention_long_bwd_workspace_bytes(R: int, n_heads: int, Tq: int, Tk: int) -> int:
    """The scratch t5_attention_long_bwd needs (rqhip_t5_attention_long_bwd_workspace_bytes): grows with
    R * n_heads * (Tq + Tk)."""
    return int(_lib.lib().rqhip_t5_attention_long_bwd_workspace_bytes(int(R), int(n_heads), int(Tq), int(Tk)))


def t5_attention_long_bwd(q: Tensor, k: Tensor, v: Tensor, out: Tensor, lse: Tensor, ml: Tensor, d_out: Tensor,
                          n_heads: int, *, bias_by_delta: Optional[Tensor] = None, bias_offset: int = 0,
                          key_mask: Optional[Tensor] = None, causal: bool = False, p: float = 0.0,
                          seed: Optional[Tensor] = None, arith: str = "fp32"):
    """The gradients of t5_attention_long_fwd_train (rqhip_t5_attention_long_bwd: a query-major launch, a key-major launch
    and, with a bias table, a small reduction) -> (dq [R, Tq, inner], dk, dv [R, Tk, inner], dtable [n_delta, n_heads] or
    None).  The arguments are the forward's, its `out`, `lse` and `ml`, and d_out [R, Tq, inner]; the weights and the
    dropout decisions are recomputed, nothing of size Tq x Tk is stored.  arith: the forward's ("fp32", or "bf16":
    rqhip_t5_attention_long_bwd_bf16)."""
    fn, fn_name = _arith_entry("t5_attention_long_bwd", arith)
    _need_gpu(q, k, v, out, lse, ml, d_out, bias_by_delta, key_mask, seed)
    q, k, v, bias_by_delta, key_mask, R, Rk, Tq, Tk, inner, seed_ptr, _, _ = _attention_args(
        "t5_attention_long_bwd", q, k, v, n_heads, bias_by_delta, key_mask, p, seed)
    out, d_out, lse, ml = _attention_bwd_args("t5_attention_long_bwd", q, out, d_out, lse, (R, int(n_heads), Tq), ml)
    with torch.cuda.device(q.device):
        ws_bytes = t5_attention_long_bwd_workspace_bytes(R, n_heads, Tq, Tk)
        dq, dk, dv, dtable, ws = _attention_grads(q, k, bias_by_delta, ((ws_bytes + 3) // 4,))
        rc = fn(_ptr(q), int(q.stride(1)), _ptr(k), _ptr(v), int(k.stride(1)), _ptr(out), int(out.stride(1)), _ptr(lse),
                _ptr(ml), _ptr(d_out), int(d_out.stride(1)), R, Rk, int(n_heads), 64, Tq, Tk, _ptr(bias_by_delta),
                0 if bias_by_delta is None else bias_by_delta.shape[0], int(bias_offset), _ptr(key_mask),
                int(bool(causal)), float(p), seed_ptr, _ptr(dq), _ptr(dk), _ptr(dv), _ptr(dtable), _ptr(ws), ws_bytes,
                _stream())
        check(rc, fn_name)
    return dq, dk, dv, dtable


def t5_add_norm_supported(dtype: torch.dtype, d: int) -> bool:
    """Whether t5_add_norm_fwd / t5_add_norm_bwd implement rows of this width (rqhip_t5_add_norm_supported): fp32, d a
    multiple of 4 in 4 .. 1024."""
    return dtype == torch.float32 and bool(_lib.lib().rqhip_t5_add_norm_supported(int(d)))


def _norm_rows(t: Optional[Tensor], name: str, who: str, shape=None) -> Optional[Tensor]:
    """A float32 [..., d] tensor as dense 16-byte-aligned rows, as the kernels' float4 accesses need them (copies when
    it is not contiguous, or is a view that starts off a 16-byte boundary); `shape`: what it must match."""
    if t is None:
        return None
    if t.dtype != torch.float32 or t.dim() < 1:
        raise RqHipError(f"{who}: {name} must be a float32 [..., d] tensor, got {t.dtype} {tuple(t.shape)}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RqHipError(f"{who}: {name} {tuple(t.shape)} does not match {tuple(shape)}")
    return _aligned16(t.contiguous())


def _aligned16(t: Tensor) -> Tensor:
    return t.clone() if t.data_ptr() % 16 else t


def _norm_call(who: str, d: int, w: Tensor, p_in: float, p_out: float, seed: Optional[Tensor]):
    """The checks t5_add_norm_fwd and t5_add_norm_bwd share -> (w as the kernels read it, the seed pointer)."""
    if w.dtype != torch.float32 or tuple(w.shape) != (d,):
        raise RqHipError(f"{who}: w must be float32 [{d}], got {w.dtype} {tuple(w.shape)}")
    return _aligned16(w.contiguous()), _dropout_seed(who, seed, p_in=p_in, p_out=p_out)


def t5_add_norm_fwd(x: Optional[Tensor], y: Tensor, w: Tensor, eps: float, p_in: float = 0.0, p_out: float = 0.0,
                    seed: Optional[Tensor] = None):
    """The tail of one T5 sub-layer and the head of the next in one launch (rqhip_t5_add_norm_fwd) -> (x_new, n, rstd):
    x_new = x + dropout(y, p_in) (x None: dropout(y, p_in)), rstd = rsqrt(mean(x_new^2) + eps) per row, n = w * (x_new *
    rstd), dropped with p_out behind a final norm.  x, y [..., d] float32, w [d]; x_new and n have y's shape, rstd
    y.shape[:-1].  The masks are t5_attention_dropout_keep(seed, 2, 1, N, d, p)[0 / 1] over the N = y.numel() / d rows;
    `seed` is a one-element int64 device tensor the host never reads."""
    _need_gpu(x, y, w, seed)
    y = _norm_rows(y, "y", "t5_add_norm_fwd")
    x = _norm_rows(x, "x", "t5_add_norm_fwd", y.shape)
    d = y.shape[-1]
    w, seed_ptr = _norm_call("t5_add_norm_fwd", d, w, p_in, p_out, seed)
    N = y.numel() // d if d else 0
    dev = y.device
    with torch.cuda.device(dev):
        x_new, n = torch.empty_like(y), torch.empty_like(y)
        rstd = torch.empty(y.shape[:-1], dtype=torch.float32, device=dev)
        rc = _lib.lib().rqhip_t5_add_norm_fwd(_ptr(x), _ptr(y), _ptr(w), N, d, float(eps), float(p_in), float(p_out),
                                              seed_ptr, _ptr(x_new), _ptr(n), _ptr(rstd), _stream())
        check(rc, "rqhip_t5_add_norm_fwd")
    return x_new, n, rstd


def t5_add_norm_bwd(x_new: Tensor, rstd: Tensor, w: Tensor, d_n: Optional[Tensor], d_xnew: Optional[Tensor],
                    p_in: float = 0.0, p_out: float = 0.0, seed: Optional[Tensor] = None, *, need_x: bool = True,
                    need_y: bool = True):
    """The gradients of t5_add_norm_fwd in one call (rqhip_t5_add_norm_bwd: one launch and the small reduction of the
    weight gradient) -> (d_x, d_y, d_w).  d_n and d_xnew are the gradients of n and x_new (None = zero); d_x / d_y are
    None when not needed, and the SAME tensor at p_in = 0, where they are equal.  d_w [d] is summed without atomics in an
    order that depends on the shape alone."""
    _need_gpu(x_new, rstd, w, d_n, d_xnew, seed)
    who = "t5_add_norm_bwd"
    x_new = _norm_rows(x_new, "x_new", who)
    d_n, d_xnew = _norm_rows(d_n, "d_n", who, x_new.shape), _norm_rows(d_xnew, "d_xnew", who, x_new.shape)
    d = x_new.shape[-1]
    w, seed_ptr = _norm_call(who, d, w, p_in, p_out, seed)
    rstd = _f32c(rstd, "rstd")
    if tuple(rstd.shape) != tuple(x_new.shape[:-1]):
        raise RqHipError(f"{who}: rstd must be {tuple(x_new.shape[:-1])}, got {tuple(rstd.shape)}")
    N = x_new.numel() // d if d else 0
    dev = x_new.device
    with torch.cuda.device(dev):
        shared = p_in == 0 and need_x and need_y
        d_x = torch.empty_like(x_new) if need_x else None
        d_y = torch.empty_like(x_new) if need_y and not shared else None
        d_w = torch.empty_like(w)
        nbytes = int(_lib.lib().rqhip_t5_add_norm_bwd_workspace_bytes(N, d))
        work = torch.empty((max(nbytes, 4) // 4,), dtype=torch.float32, device=dev)
        rc = _lib.lib().rqhip_t5_add_norm_bwd(_ptr(x_new), _ptr(rstd), _ptr(w), _ptr(d_n), _ptr(d_xnew), N, d, float(p_in),
                                              float(p_out), seed_ptr, _ptr(d_x), _ptr(d_y), _ptr(d_w), _ptr(work), nbytes,
                                              _stream())
        check(rc, "rqhip_t5_add_norm_bwd")
    return d_x, (d_x if shared else d_y), d_w


def t5_ffn_supported(dtype: torch.dtype, d: int, F: int) -> bool:
    """Whether t5_ffn_fwd / t5_ffn_bwd implement this (d_model, d_ff) (rqhip_t5_ffn_supported): fp32, d a multiple of 32
    in 32 .. 512, F a multiple of 32 in 32 .. 8192."""
    return dtype == torch.float32 and bool(_lib.lib().rqhip_t5_ffn_supported(int(d), int(F)))


def _ffn_call(who: str, x: Tensor, wi: Tensor, wo: Tensor, p: float, seed: Optional[Tensor]):
    """The checks and copies t5_ffn_fwd and t5_ffn_bwd share -> (x, wi, wo as the kernels read them, N, d, F, seed pointer)."""
    x = _norm_rows(x, "x", who)
    d = x.shape[-1]
    if wi.dtype != torch.float32 or wi.dim() != 2 or wi.shape[1] != d:
        raise RqHipError(f"{who}: wi must be float32 [F, {d}], got {wi.dtype} {tuple(wi.shape)}")
    F = wi.shape[0]
    if wo.dtype != torch.float32 or tuple(wo.shape) != (d, F):
        raise RqHipError(f"{who}: wo must be float32 [{d}, {F}], got {wo.dtype} {tuple(wo.shape)}")
    seed_ptr = _dropout_seed(who, seed, p=p)
    if not t5_ffn_supported(x.dtype, d, F):
        raise RqHipError(f"{who}: (d, F) = ({d}, {F}) is not supported (multiples of 32, d <= 512, F <= 8192)")
    return x, _aligned16(wi.contiguous()), _aligned16(wo.contiguous()), (x.numel() // d), d, F, seed_ptr


def t5_act_image_numel(N: int, C: int) -> int:
    """bf16 elements of the blocked image of an [N, C] activation (rqhip_t5_ffn_act_image_bytes): 32 * ceil(N / 32) * C."""
    return int(_lib.lib().rqhip_t5_ffn_act_image_bytes(int(N), int(C))) // 2


def t5_act_image_rows(img: Tensor, N: int, C: int) -> Tensor:
    """The row-major [N, C] bfloat16 tensor of a blocked activation image (include/rqhip.h: element (n, c) is number
    ((n >> 5) * C + c) * 32 + 8 * (n & 3) + ((n & 31) >> 2) of the buffer).  An index permutation in torch operators, on
    the image's device: for tests and for looking inside an image, not for a hot path."""
    N, C = int(N), int(C)
    nb = (N + 31) // 32
    if C < 32 or C % 32 or img.dtype != torch.bfloat16 or img.numel() != nb * C * 32:
        raise RqHipError(f"t5_act_image_rows: an image of [{N}, {C}] is {nb * C * 32} bfloat16 with C a multiple of 32, got "
                         f"{img.dtype} {tuple(img.shape)}")
    # buffer [b, c, kq, ks] -> rows [b, ks, kq] (rho = 4 ks + kq), columns c
    return img.reshape(nb, C, 4, 8).permute(0, 3, 2, 1).reshape(nb * 32, C)[:N].contiguous()


def _act_image(who: str, img, name: str, N: int, C: int, dev) -> Tensor:
    """A blocked activation image as the kernels read it: a dense, 16-byte aligned bfloat16 tensor of its size on `dev`."""
    n = 32 * ((N + 31) // 32) * C
    if not isinstance(img, Tensor) or img.dtype != torch.bfloat16 or img.numel() != n or img.device != dev:
        got = f"{img.dtype} {tuple(img.shape)} on {img.device}" if isinstance(img, Tensor) else repr(type(img))
        raise RqHipError(f"{who}: {name} must be a bfloat16 image of {n} elements on {dev} (t5_ffn_fwd, saved=\"bf16\"), got {got}")
    if not img.is_contiguous() or img.data_ptr() % 16:
        raise RqHipError(f"{who}: {name} must be dense and 16-byte aligned")
    return img


def _ffn_grads(like: Tensor, N: int, d: int, F: int, need_x: bool, need_wi: bool, need_wo: bool):
    """The outputs of a feed-forward backward -> (d_x of `like`'s shape, d_wi [F, d], d_wo [d, F]), None where not needed."""
    make = torch.zeros if N == 0 else torch.empty      # without rows the sums are empty
    return (torch.empty_like(like) if need_x else None,
            make((F, d), dtype=torch.float32, device=like.device) if need_wi else None,
            make((d, F), dtype=torch.float32, device=like.device) if need_wo else None)


def t5_ffn_fwd(x: Tensor, wi: Tensor, wo: Tensor, p: float = 0.0, seed: Optional[Tensor] = None, *, need_h: bool = True,
               arith: str = "fp32", w_images=None, saved: str = "fp32"):
    """The T5 feed-forward body in one launch (rqhip_t5_ffn_fwd) -> (y, h or None): h = relu(x @ wi.T), y = dropout(h, p)
    @ wo.T.  x [..., d] float32, wi [F, d] and wo [d, F] the two Linear weights as stored; y has x's shape, h is
    [..., F] (the one tensor t5_ffn_bwd needs; not stored without need_h).  The mask is t5_attention_dropout_keep(seed,
    1, 1, N, F, p)[0, 0] over the N = x.numel() / d rows; `seed` is a one-element int64 device tensor the host never
    reads.  arith: "fp32", or "bf16" (rqhip_t5_ffn_fwd_bf16: every matrix operand rounded to bf16, fp32 accumulation;
    all tensors stay float32 and h is stored unrounded).  w_images (arith "bf16" only): the pair (wi16 [F, d], wo16 [d,
    F]) of bf16 images of wi and wo (bf16_images); the kernel reads them instead of the weights, and every result has
    the bits of the call without them (rqhip_t5_ffn_fwd_bf16w).  saved (T5_SAVED; "bf16" with arith "bf16" only, with or
    without w_images): with "bf16" the second result is the pair (hd16, x16) of blocked bf16 images (t5_act_image_rows) of
    dropout(h) and of x, all that t5_ffn_bwd then needs of the activations (rqhip_t5_ffn_fwd_bf16a / _bf16wa); y keeps
    its bits.  Without need_h the second result is None either way."""
    who = "t5_ffn_fwd"
    _, fn, fn_name = t5_matmul_entry(who, arith, w_images, saved)
    _need_gpu(x, wi, wo, seed)
    x, wi, wo, N, d, F, seed_ptr = _ffn_call(who, x, wi, wo, p, seed)
    dev = x.device
    if w_images is not None:
        wi16, wo16 = w_images
        wi, wo = _image(who, wi16, "w_images[0]", (F, d), dev), _image(who, wo16, "w_images[1]", (d, F), dev)
    with torch.cuda.device(dev):
        y = torch.empty_like(x)
        if saved == "bf16":
            hd16 = torch.empty((t5_act_image_numel(N, F),), dtype=torch.bfloat16, device=dev) if need_h else None
            x16 = torch.empty((t5_act_image_numel(N, d),), dtype=torch.bfloat16, device=dev) if need_h else None
            rc = fn(_ptr(x), _ptr(wi), _ptr(wo), N, d, F, float(p), seed_ptr, _ptr(y), _ptr(hd16), _ptr(x16), _stream())
            check(rc, fn_name)
            return y, ((hd16, x16) if need_h else None)
        h = torch.empty(x.shape[:-1] + (F,), dtype=torch.float32, device=dev) if need_h else None
        rc = fn(_ptr(x), _ptr(wi), _ptr(wo), N, d, F, float(p), seed_ptr, _ptr(y), _ptr(h), _stream())
        check(rc, fn_name)
    return y, h


def t5_ffn_bwd(x: Tensor, wi: Tensor, wo: Tensor, h: Tensor, d_y: Tensor, p: float = 0.0, seed: Optional[Tensor] = None, *,
               need_x: bool = True, need_wi: bool = True, need_wo: bool = True, return_g: bool = False,
               arith: str = "fp32", w_images=None, saved: str = "fp32"):
    """The gradients of t5_ffn_fwd in one call of at most two launches (rqhip_t5_ffn_bwd) -> (d_x, d_wi, d_wo), None
    where not needed.  x, wi, wo, p, seed: the forward's; h: its second result; d_y: the gradient of y.  The dropout
    decisions are recomputed from the seed; the weight gradients are summed without atomics in an order that depends on
    the shape alone.  The [N, F] workspace comes from torch's allocator.  return_g: a fourth result, the workspace as the
    tensor g of h's shape when need_wi (else None).  arith: "fp32" or "bf16", as t5_ffn_fwd's (rqhip_t5_ffn_bwd_bf16).
    w_images (arith "bf16" only): the pair (wi16t [d, F], wo16t [F, d]) of TRANSPOSED bf16 images of wi and wo, which
    this call reads instead of the weights; the bits are those of the call without them (rqhip_t5_ffn_bwd_bf16w).
    saved="bf16" (arith "bf16" only): x is None and h is the forward's pair (hd16, x16); no seed is read, the active set
    is hd16 > 0, the workspace holds bf16 images of d_y and g, and every gradient has the bits of the call on the fp32 h
    (rqhip_t5_ffn_bwd_bf16a / _bf16wa); return_g then gives g as the row-major bfloat16 tensor of its image."""
    who = "t5_ffn_bwd"
    _, fn, fn_name = t5_matmul_entry(who, arith, w_images, saved)
    if saved == "bf16":
        return _ffn_bwd_saved(who, fn, fn_name, wi, wo, h, d_y, p, need_x, need_wi, need_wo, return_g, w_images)
    _need_gpu(x, wi, wo, h, d_y, seed)
    x, wi, wo, N, d, F, seed_ptr = _ffn_call(who, x, wi, wo, p, seed)
    if w_images is not None:
        wi16t, wo16t = w_images
        wi = _image(who, wi16t, "w_images[0]", (d, F), x.device)
        wo = _image(who, wo16t, "w_images[1]", (F, d), x.device)
    h = _norm_rows(h, "h", who, x.shape[:-1] + (F,))
    d_y = _norm_rows(d_y, "d_y", who, x.shape)
    dev = x.device
    with torch.cuda.device(dev):
        d_x, d_wi, d_wo = _ffn_grads(x, N, d, F, need_x, need_wi, need_wo)
        work = None
        if need_wi and N > 0:
            nbytes = int(_lib.lib().rqhip_t5_ffn_bwd_workspace_bytes(N, d, F))
            work = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev)
        rc = fn(_ptr(x), _ptr(wi), _ptr(wo), _ptr(h), _ptr(d_y), N, d, F, float(p), seed_ptr, _ptr(d_x), _ptr(d_wi),
                _ptr(d_wo), _ptr(work), _stream())
        check(rc, fn_name)
    if return_g:
        return d_x, d_wi, d_wo, (work.view(h.shape) if work is not None else None)
    return d_x, d_wi, d_wo


def _ffn_bwd_saved(who, fn, fn_name, wi, wo, pair, d_y, p, need_x, need_wi, need_wo, return_g, w_images):
    """t5_ffn_bwd on bf16 saved activations: `pair` is the forward's (hd16, x16)."""
    if not isinstance(pair, (tuple, list)) or len(pair) != 2:
        raise RqHipError(f'{who}: with saved="bf16", h is the pair (hd16, x16) of t5_ffn_fwd(..., saved="bf16")')
    hd16, x16 = pair
    _need_gpu(wi, wo, hd16, x16, d_y)
    if not 0.0 <= p < 1.0:
        raise RqHipError(f"{who}: p={p} outside 0 <= p < 1")
    d_y, wi, wo, N, d, F, _ = _ffn_call(who, d_y, wi, wo, 0.0, None)    # d_y has x's shape and checks; no seed is read
    dev = d_y.device
    if w_images is not None:
        wi16t, wo16t = w_images
        wi, wo = _image(who, wi16t, "w_images[0]", (d, F), dev), _image(who, wo16t, "w_images[1]", (F, d), dev)
    hd16, x16 = _act_image(who, hd16, "hd16", N, F, dev), _act_image(who, x16, "x16", N, d, dev)
    with torch.cuda.device(dev):
        d_x, d_wi, d_wo = _ffn_grads(d_y, N, d, F, need_x, need_wi, need_wo)
        work = None
        if (need_wi or need_wo) and N > 0:      # dy16, and behind it g16 when d_wi is wanted
            n = t5_act_image_numel(N, d) + (t5_act_image_numel(N, F) if need_wi else 0)
            work = torch.empty((n,), dtype=torch.bfloat16, device=dev)
        rc = fn(_ptr(x16), _ptr(wi), _ptr(wo), _ptr(hd16), _ptr(d_y), N, d, F, float(p), _ptr(d_x), _ptr(d_wi), _ptr(d_wo),
                _ptr(work), _stream())
        check(rc, fn_name)
    if return_g:
        g = None
        if work is not None and need_wi:
            g = t5_act_image_rows(work[t5_act_image_numel(N, d):], N, F).view(d_y.shape[:-1] + (F,))
        return d_x, d_wi, d_wo, g
    return d_x, d_wi, d_wo


T5_PROJ_MAX_GROUP = 8   # weights per t5_proj_fwd / t5_proj_bwd call


def t5_proj_supported(dtype: torch.dtype, d_in: int, d_out: int, n: int = 1) -> bool:
    """Whether t5_proj_fwd / t5_proj_bwd implement a group of n [d_out, d_in] weights (rqhip_t5_proj_supported): fp32,
    d_in and d_out multiples of 32 in 32 .. 512, 1 <= n <= 8."""
    return dtype == torch.float32 and bool(_lib.lib().rqhip_t5_proj_supported(int(d_in), int(d_out), int(n)))


def _proj_call(who: str, x: Tensor, weights, w_images=None, image_shape=None):
    """The checks and copies t5_proj_fwd and t5_proj_bwd share -> (x as dense aligned rows, the weights as the kernels
    read them, their HOST pointer array, N, d_in, d_out).  w_images: one bf16 image per weight, whose pointers then
    stand in the array; image_shape(d_out, d_in) is the shape of each."""
    weights = list(weights)
    _need_gpu(x, *weights)
    x = _norm_rows(x, "x", who)
    d_in, n = x.shape[-1], len(weights)
    d_out = weights[0].shape[0] if n and weights[0].dim() == 2 else -1
    for j, w in enumerate(weights):
        if w.dtype != torch.float32 or tuple(w.shape) != (d_out, d_in):
            raise RqHipError(f"{who}: weights[{j}] must be float32 [d_out, {d_in}] like weights[0], got {w.dtype} "
                             f"{tuple(w.shape)}")
    if not t5_proj_supported(x.dtype, d_in, d_out, n):
        raise RqHipError(f"{who}: (d_in, d_out, n) = ({d_in}, {d_out}, {n}) is not supported (multiples of 32 up to 512, "
                         f"1 <= n <= 8)")
    if w_images is not None:
        w_images = list(w_images)
        if len(w_images) != n:
            raise RqHipError(f"{who}: {len(w_images)} w_images for {n} weights")
        weights = [_image(who, img, f"w_images[{j}]", image_shape(d_out, d_in), x.device)
                   for j, img in enumerate(w_images)]
    else:
        weights = [_aligned16(w.contiguous()) for w in weights]
    w_ptrs = (C.c_void_p * n)(*[w.data_ptr() for w in weights])
    return x, weights, w_ptrs, (x.numel() // d_in), d_in, d_out


def t5_proj_fwd(x: Tensor, weights, outs=None, *, arith: str = "fp32", w_images=None):
    """n bias-free linear maps of the same rows in one launch (rqhip_t5_proj_fwd) -> (y[0], ..., y[n - 1]), y[j] = x @
    weights[j].T.  x [..., d_in] float32 with dense rows, weights: n separate [d_out, d_in] matrices, the nn.Linear
    weights as stored.  y[j] has shape x.shape[:-1] + (d_out,).  outs (optional): a list of n entries, each None (that
    output is allocated) or a preallocated float32 [N, d_out] view over the N = x.numel() / d_in rows whose last
    dimension is dense and whose row stride is at least d_out, a position of a decode-cache slab for one; the kernel
    writes into it and it is returned as it is.  arith: "fp32", or "bf16" (rqhip_t5_proj_fwd_bf16: x and the weights
    rounded to bf16 as operands, fp32 accumulation; all tensors stay float32).  w_images (arith "bf16" only): n bf16
    images [d_out, d_in] of the weights (bf16_images), read instead of them; the bits are those of the call without
    them (rqhip_t5_proj_fwd_bf16w)."""
    who = "t5_proj_fwd"
    _, fn, fn_name = t5_matmul_entry(who, arith, w_images)
    x, weights, w_ptrs, N, d_in, d_out = _proj_call(who, x, weights, w_images, lambda o, i: (o, i))
    n = len(weights)
    outs = [None] * n if outs is None else list(outs)
    if len(outs) != n:
        raise RqHipError(f"{who}: {len(outs)} outs for {n} weights")
    dev = x.device
    with torch.cuda.device(dev):
        for j, o in enumerate(outs):
            if o is None:
                outs[j] = torch.empty(x.shape[:-1] + (d_out,), dtype=torch.float32, device=dev)
            elif (o.dtype != torch.float32 or o.device != dev or tuple(o.shape) != (N, d_out)
                  or (N > 0 and o.stride(1) != 1) or (N > 1 and o.stride(0) < d_out)):
                raise RqHipError(f"{who}: outs[{j}] must be a float32 [{N}, {d_out}] view on {dev} with dense rows at "
                                 f"least {d_out} apart, got {o.dtype} {tuple(o.shape)} strides {tuple(o.stride())}")
        y_ptrs = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
        ld_y = (C.c_int64 * n)(*[int(o.stride(0)) if o.dim() == 2 and N > 1 else d_out for o in outs])
        rc = fn(_ptr(x), d_in, w_ptrs, y_ptrs, ld_y, n, N, d_in, d_out, _stream())
        check(rc, fn_name)
    return tuple(outs)


def t5_proj_bwd(x: Tensor, weights, d_ys, need_x: bool = True, need_w=None, *, arith: str = "fp32", w_images=None):
    """The gradients of t5_proj_fwd in one call of at most two launches (rqhip_t5_proj_bwd) -> (d_x, [d_w[0], ...]).
    d_ys: n upstream gradients, each of y[j]'s shape or None; a None contributes nothing to d_x and gets no d_w[j].  d_x
    (x's shape) is None without need_x or when every d_ys[j] is None; d_w[j] is None where need_w[j] (default: every
    weight) is false.  No atomics: the same bits on every run.  arith: "fp32" or "bf16", as t5_proj_fwd's
    (rqhip_t5_proj_bwd_bf16).  w_images (arith "bf16" only): n TRANSPOSED bf16 images [d_in, d_out] of the weights,
    read instead of them; the bits are those of the call without them (rqhip_t5_proj_bwd_bf16w)."""
    who = "t5_proj_bwd"
    _, fn, fn_name = t5_matmul_entry(who, arith, w_images)
    shape = x.shape
    x, weights, w_ptrs, N, d_in, d_out = _proj_call(who, x, weights, w_images, lambda o, i: (i, o))
    n = len(weights)
    d_ys = list(d_ys)
    need_w = [True] * n if need_w is None else [bool(f) for f in need_w]
    if len(d_ys) != n or len(need_w) != n:
        raise RqHipError(f"{who}: {len(d_ys)} d_ys and {len(need_w)} need_w for {n} weights")
    _need_gpu(*d_ys)
    d_ys = [_norm_rows(g, f"d_ys[{j}]", who, tuple(shape[:-1]) + (d_out,)) for j, g in enumerate(d_ys)]
    live = any(g is not None for g in d_ys)
    dev = x.device
    with torch.cuda.device(dev):
        d_x = torch.empty_like(x) if need_x and live else None
        make = torch.zeros if N == 0 else torch.empty      # without rows the sums are empty
        d_w = [make((d_out, d_in), dtype=torch.float32, device=dev) if f and g is not None else None
               for f, g in zip(need_w, d_ys)]
        g_ptrs = (C.c_void_p * n)(*[_ptr(g) for g in d_ys])
        ld_dy = (C.c_int64 * n)(*([d_out] * n))
        dw_ptrs = (C.c_void_p * n)(*[_ptr(g) for g in d_w])
        rc = fn(_ptr(x), d_in, w_ptrs, g_ptrs, ld_dy, n, N, d_in, d_out, _ptr(d_x), dw_ptrs, _stream())
        check(rc, fn_name)
    return d_x, d_w


class Bf16ImageJobs(NamedTuple):
    """What one bf16_images launch needs: the job table in device memory, its job and tile counts, and the tensors the
    table points at (kept alive with it)."""
    table: Tensor
    n_jobs: int
    n_tiles: int
    tensors: tuple


def bf16_images_alloc(weights, transposed: bool = True):
    """Room for the bf16 images of `weights` (float32 [rows, cols] device matrices, both multiples of 32) -> (arena, imgs,
    imgs_t): ONE bfloat16 allocation and, as views of it, an image [rows, cols] per weight and, with `transposed`, its
    transpose [cols, rows] (else imgs_t is a list of None).  Nothing is computed: bf16_images fills them."""
    weights = list(weights)
    dev = _need_gpu(*weights)
    for j, w in enumerate(weights):
        if w.dtype != torch.float32 or w.dim() != 2 or w.shape[0] % 32 or w.shape[1] % 32 or not w.numel():
            raise RqHipError(f"bf16_images_alloc: weights[{j}] must be a float32 matrix whose sizes are multiples of 32, "
                             f"got {w.dtype} {tuple(w.shape)}")
    per = 2 if transposed else 1
    with torch.cuda.device(dev):
        arena = torch.empty((per * sum(w.numel() for w in weights),), dtype=torch.bfloat16, device=dev)
    imgs, imgs_t, at = [], [], 0
    for w in weights:      # every view starts a multiple of 1024 elements into the arena: 16-byte aligned
        r, c = w.shape
        imgs.append(arena[at:at + r * c].view(r, c))
        at += r * c
        imgs_t.append(arena[at:at + r * c].view(c, r) if transposed else None)
        at += r * c if transposed else 0
    return arena, imgs, imgs_t


def bf16_images_jobs(weights, imgs, imgs_t=None) -> Bf16ImageJobs:
    """The device job table of one bf16_images launch over `weights` (rqhip_bf16_images_fill_jobs, then ONE copy to the
    device).  weights[j]: a dense, 16-byte aligned float32 [rows, cols] device matrix, read in place; imgs[j] / imgs_t[j]:
    its bfloat16 image [rows, cols] and transposed image [cols, rows] (imgs_t, or an entry of it, None: not made).  The
    table holds POINTERS: build it again when a weight or an image moves."""
    who = "bf16_images_jobs"
    weights, imgs = list(weights), list(imgs)
    n = len(weights)
    imgs_t = [None] * n if imgs_t is None else list(imgs_t)
    if len(imgs) != n or len(imgs_t) != n:
        raise RqHipError(f"{who}: {len(imgs)} imgs and {len(imgs_t)} imgs_t for {n} weights")
    dev = _need_gpu(*weights, *imgs, *imgs_t)
    for j, w in enumerate(weights):
        if w.dtype != torch.float32 or w.dim() != 2 or not w.is_contiguous():
            raise RqHipError(f"{who}: weights[{j}] must be a dense float32 matrix, got {w.dtype} {tuple(w.shape)}")
        _image(who, imgs[j], f"imgs[{j}]", w.shape, dev)
        if imgs_t[j] is not None:
            _image(who, imgs_t[j], f"imgs_t[{j}]", (w.shape[1], w.shape[0]), dev)
    l = _lib.lib()
    vp = C.c_void_p * n
    host = torch.empty((max(int(l.rqhip_bf16_images_job_bytes(n)), 1),), dtype=torch.uint8)
    n_tiles = C.c_int64(0)
    rc = l.rqhip_bf16_images_fill_jobs(host.data_ptr(), vp(*[w.data_ptr() for w in weights]),
                                       vp(*[t.data_ptr() for t in imgs]), vp(*[_ptr(t) for t in imgs_t]),
                                       (C.c_int64 * n)(*[w.shape[0] for w in weights]),
                                       (C.c_int64 * n)(*[w.shape[1] for w in weights]), n, C.byref(n_tiles))
    check(rc, "rqhip_bf16_images_fill_jobs")
    table = host.to(dev) if n else host
    return Bf16ImageJobs(table, n, int(n_tiles.value), (tuple(weights), tuple(imgs), tuple(imgs_t)))


def bf16_images(jobs: Bf16ImageJobs) -> None:
    """Make (or refresh) the bf16 images of a job table in ONE launch (rqhip_bf16_images): imgs[j] = the weights rounded
    to bf16, nearest even, the very operands the "bf16" arithmetic forms in registers, and imgs_t[j] their transposes.
    No copy, allocation or host read: the call can be captured into a graph."""
    if jobs.n_jobs == 0:
        return
    dev = jobs.table.device
    with torch.cuda.device(dev):
        check(_lib.lib().rqhip_bf16_images(jobs.table.data_ptr(), jobs.n_jobs, jobs.n_tiles, _stream()), "rqhip_bf16_images")


def sid_head_loss_supported(dtype: torch.dtype, d: int, K: int, L: int) -> bool:
    """Whether sid_head_loss_fwd / sid_head_loss_bwd implement this shape (rqhip_sid_head_loss_supported): fp32, d a
    multiple of 4 in 4 .. 1024, K in 1 .. 1024 codes, L in 1 .. 8 levels."""
    return dtype == torch.float32 and bool(_lib.lib().rqhip_sid_head_loss_supported(int(d), int(K), int(L)))


def _sid_head_args(who: str, x: Tensor, weights, target: Tensor, L: int):
    """The checks sid_head_loss_fwd and sid_head_loss_bwd share -> (x, its two strides, the weights' pointer array,
    target, its row stride, B, T, K, d).  x and target go to the kernels as strided views; only a layout the kernels
    cannot address (a last dimension that is not dense, strides off a float4 boundary) is copied."""
    weights = list(weights)
    _need_gpu(x, target, *weights)
    L = int(L)
    if x.dtype != torch.float32 or x.dim() != 3:
        raise RqHipError(f"{who}: x must be a float32 [B, T, d] tensor, got {x.dtype} {tuple(x.shape)}")
    B, T, d = x.shape
    if len(weights) != L or L < 1:
        raise RqHipError(f"{who}: {len(weights)} weight matrices for L={L} levels")
    K = weights[0].shape[0] if weights[0].dim() == 2 else -1
    for h, w in enumerate(weights):
        if w.dtype != torch.float32 or tuple(w.shape) != (K, d):
            raise RqHipError(f"{who}: weights[{h}] must be float32 [K, {d}] like weights[0], got {w.dtype} {tuple(w.shape)}")
    if target.dim() != 2 or target.shape[0] != B or target.shape[1] < L or target.is_floating_point():
        raise RqHipError(f"{who}: target must be an integer [{B}, >= {L}] tensor, got {target.dtype} {tuple(target.shape)}")
    if target.dtype != torch.int64:
        target = target.long()
    if target.stride(1) != 1 or target.stride(0) < L:
        target = target.contiguous()
    if x.stride(2) != 1 or x.stride(0) < 0 or x.stride(1) < 0 or x.stride(0) % 4 or x.stride(1) % 4 or x.data_ptr() % 16:
        x = _aligned16(x.contiguous())
    weights = [_aligned16(w.contiguous()) for w in weights]
    w_ptrs = (C.c_void_p * L)(*[w.data_ptr() for w in weights])
    return x, int(x.stride(0)), int(x.stride(1)), weights, w_ptrs, target, int(target.stride(0)), B, T, K, d


def sid_head_loss_fwd(x: Tensor, weights, target: Tensor, L: int):
    """All L semantic-id heads and their cross-entropy losses in one call (rqhip_sid_head_loss_fwd) ->
    (loss, loss_d, z, lse): z[b, h] = weights[h] @ x[b, h], loss_d[h] = mean_b cross_entropy(z[:, h], target[:, h]),
    loss = their sum in ascending order from 0.  x [B, T >= L, d] float32 (any row and position strides that are
    multiples of 4; positions >= L are never read), weights: L separate [K, d] matrices, target [B, >= L] integers
    (converted to int64 when they are not; columns >= L are never read).  loss is 0-dim, loss_d [L]; z [B, L, K] and
    lse [B, L] are what sid_head_loss_bwd needs.  A target outside [0, K) makes its level's loss NaN; there is no
    ignore_index."""
    who = "sid_head_loss_fwd"
    x, ld_xb, ld_xt, weights, w_ptrs, target, ld_t, B, T, K, d = _sid_head_args(who, x, weights, target, L)
    dev = x.device
    with torch.cuda.device(dev):
        z = torch.empty((B, L, K), dtype=torch.float32, device=dev)
        rows = torch.empty((2, B, L), dtype=torch.float32, device=dev)    # lse [B, L]; the rows' losses [L, B]
        loss_d = torch.empty((L,), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        rc = _lib.lib().rqhip_sid_head_loss_fwd(_ptr(x), ld_xb, ld_xt, w_ptrs, _ptr(target), ld_t, B, T, int(L), K, d,
                                                _ptr(z), _ptr(rows[0]), _ptr(rows[1]), _ptr(loss_d), _ptr(loss), _stream())
        check(rc, "rqhip_sid_head_loss_fwd")
    return loss, loss_d, z, rows[0]


def sid_head_loss_bwd(x: Tensor, weights, target: Tensor, z: Tensor, lse: Tensor, d_loss: Tensor, L: int, *,
                      need_x: bool = True, need_w=None):
    """The gradients of sid_head_loss_fwd's `loss` in one launch (rqhip_sid_head_loss_bwd) -> (d_x, [d_w[0], ...]).
    z, lse: the forward's; d_loss: the upstream gradient, a one-element float32 device tensor the host never reads.
    d_x is a dense [B, T, d] tensor whose positions >= L are zero (None without need_x); d_w[h] is None where need_w[h]
    (default: every level) is false.  No atomics: the same bits on every run."""
    who = "sid_head_loss_bwd"
    x, ld_xb, ld_xt, weights, w_ptrs, target, ld_t, B, T, K, d = _sid_head_args(who, x, weights, target, L)
    L = int(L)
    need_w = [True] * L if need_w is None else [bool(n) for n in need_w]
    _need_gpu(z, lse, d_loss)
    z, lse = _f32c(z, "z"), _f32c(lse, "lse")
    if tuple(z.shape) != (B, L, K) or tuple(lse.shape) != (B, L) or len(need_w) != L:
        raise RqHipError(f"{who}: z {tuple(z.shape)}, lse {tuple(lse.shape)}, need_w {len(need_w)} do not match "
                         f"B={B}, L={L}, K={K}")
    if d_loss.dtype != torch.float32 or d_loss.numel() != 1:
        raise RqHipError(f"{who}: d_loss must be one float32 element, got {d_loss.dtype} {tuple(d_loss.shape)}")
    dev = x.device
    with torch.cuda.device(dev):
        d_x = torch.empty((B, T, d), dtype=torch.float32, device=dev) if need_x else None
        d_w = [torch.empty((K, d), dtype=torch.float32, device=dev) if n else None for n in need_w]
        g_ptrs = (C.c_void_p * L)(*[_ptr(g) for g in d_w])
        rc = _lib.lib().rqhip_sid_head_loss_bwd(_ptr(x), ld_xb, ld_xt, w_ptrs, _ptr(target), ld_t, _ptr(z), _ptr(lse),
                                                _ptr(d_loss), B, T, L, K, d, _ptr(d_x), g_ptrs, _stream())
        check(rc, "rqhip_sid_head_loss_bwd")
    return d_x, d_w


def sid_embed_supported(dtype: torch.dtype, d: int, L: int) -> bool:
    """Whether sid_embed_fwd / sid_embed_bwd implement this shape (rqhip_sid_embed_supported): fp32, d a multiple of 4
    in 4 .. 1024, L in 1 .. 8 levels."""
    return dtype == torch.float32 and bool(_lib.lib().rqhip_sid_embed_supported(int(d), int(L)))


def _sid_embed_plan(who: str, ids: Tensor, mask: Optional[Tensor], L: int, ld_item: int, d: int,
                    prefix_idx: Optional[Tensor]):
    """The checks of the row plan sid_embed_fwd and sid_embed_bwd share (shapes and dtypes first, so that they are
    reported on any device) -> (ids, mask, its element size, B, items, prefix_idx, its row stride)."""
    L, ld_item = int(L), int(ld_item)
    if ids.dim() != 2 or ids.dtype != torch.int64:
        raise RqHipError(f"{who}: ids must be an int64 [B, items * ld_item] tensor, got {ids.dtype} {tuple(ids.shape)}")
    if L < 1 or ld_item < L or ids.shape[1] < ld_item or ids.shape[1] % ld_item:
        raise RqHipError(f"{who}: ids of width {ids.shape[1]} are not items * ld_item columns (ld_item={ld_item}, L={L})")
    if mask is not None and (mask.dtype not in (torch.bool, torch.int64) or mask.shape != ids.shape):
        raise RqHipError(f"{who}: mask must be a bool or int64 tensor of ids' shape {tuple(ids.shape)}, got {mask.dtype} "
                         f"{tuple(mask.shape)}")
    if prefix_idx is not None and (prefix_idx.dtype != torch.int64 or prefix_idx.dim() not in (1, 2)
                                   or prefix_idx.shape[0] != ids.shape[0]):
        raise RqHipError(f"{who}: prefix_idx must be an int64 [{ids.shape[0]}] or [{ids.shape[0]}, n] tensor (column 0 "
                         f"is read), got {prefix_idx.dtype} {tuple(prefix_idx.shape)}")
    if not sid_embed_supported(torch.float32, d, L):
        raise RqHipError(f"{who}: (d, L) = ({d}, {L}) is not supported (d a multiple of 4 in 4 .. 1024, L in 1 .. 8)")
    _need_gpu(ids, mask, prefix_idx)
    ids = ids.contiguous()
    if mask is not None:
        mask = mask.contiguous()
    ld_p = 0
    if prefix_idx is not None:
        if prefix_idx.shape[0] > 1 and prefix_idx.stride(0) < 1:
            prefix_idx = prefix_idx.contiguous()
        ld_p = int(prefix_idx.stride(0))
    return (ids, mask, 0 if mask is None else mask.element_size(), ids.shape[0], ids.shape[1] // ld_item, prefix_idx,
            ld_p)


def sid_embed_fwd(ids: Tensor, mask: Optional[Tensor], table: Tensor, L: int, ld_item: int, sep: Optional[Tensor] = None,
                  prefix_table: Optional[Tensor] = None, prefix_idx: Optional[Tensor] = None, *, need_mask: bool = True):
    """Semantic ids -> a T5 stack's inputs_embeds in one launch (rqhip_sid_embed_fwd) -> (x, mask_out).  Row b of x
    [B, T, d] is an optional prefix, then per item its L id positions and an optional separator, T = has_prefix + items
    * (L + has_sep):
      ids [B, items * ld_item] int64, ld_item >= L columns per item (columns >= L of an item are never read); mask None
      or a bool / int64 tensor of the same shape; table [L * K, d] float32.  Position (item i, level h) is row
      (ids[b, i * ld_item + h] + h * K) * (mask != 0) of table: a padded id (-1, mask 0) is row 0.
      sep: None or d float32 elements, the position behind each item.
      prefix_table [rows, d]: position 0 is its row remainder(prefix_idx[b] or prefix_idx[b, 0], rows), or its row 0 for
      every b without prefix_idx (a [1, d] parameter).
    mask_out [B, T] bool (None without need_mask): True at the prefix, mask != 0 at an id position and at a separator
    that of its item's last level.  x has the operators' bits: it is a gather.
    An index outside the table is never used as an address, where the operators would raise a device assert: it is
    clamped into the table here (row 0 or the last row) and its token is dropped by sid_embed_bwd."""
    who = "sid_embed_fwd"
    if table.dtype != torch.float32 or table.dim() != 2 or table.shape[0] % max(int(L), 1):
        raise RqHipError(f"{who}: table must be float32 [L * K, d] with L={L}, got {table.dtype} {tuple(table.shape)}")
    d, K = table.shape[1], table.shape[0] // max(int(L), 1)
    if sep is not None and (sep.dtype != torch.float32 or sep.numel() != d):
        raise RqHipError(f"{who}: sep must hold {d} float32 elements, got {sep.dtype} {tuple(sep.shape)}")
    if prefix_table is not None and (prefix_table.dtype != torch.float32 or prefix_table.dim() != 2
                                     or prefix_table.shape[1] != d or prefix_table.shape[0] < 1):
        raise RqHipError(f"{who}: prefix_table must be float32 [rows >= 1, {d}], got {prefix_table.dtype} "
                         f"{tuple(prefix_table.shape)}")
    if prefix_table is None:
        prefix_idx = None
    ids, mask, elt, B, items, prefix_idx, ld_p = _sid_embed_plan(who, ids, mask, L, ld_item, d, prefix_idx)
    _need_gpu(ids, table, sep, prefix_table)
    table = _aligned16(table.contiguous())
    sep = None if sep is None else _aligned16(sep.contiguous())
    prefix_table = None if prefix_table is None else _aligned16(prefix_table.contiguous())
    T = (prefix_table is not None) + items * (int(L) + (sep is not None))
    dev = ids.device
    with torch.cuda.device(dev):
        x = torch.empty((B, T, d), dtype=torch.float32, device=dev)
        mask_out = torch.empty((B, T), dtype=torch.bool, device=dev) if need_mask else None
        rc = _lib.lib().rqhip_sid_embed_fwd(_ptr(ids), _ptr(mask), elt, B, items, int(L), int(ld_item), K, d, _ptr(table),
                                            _ptr(sep), _ptr(prefix_table), _ptr(prefix_idx), ld_p,
                                            0 if prefix_table is None else prefix_table.shape[0], _ptr(x),
                                            _ptr(mask_out), _stream())
        check(rc, "rqhip_sid_embed_fwd")
    return x, mask_out


def sid_embed_bwd(d_x: Tensor, ids: Tensor, mask: Optional[Tensor], L: int, ld_item: int, K: int, *, has_sep: bool,
                  prefix_rows: int = 0, prefix_idx: Optional[Tensor] = None, need_table: bool = True,
                  need_sep: bool = True, need_prefix: bool = True):
    """The gradients of sid_embed_fwd's x in one launch (rqhip_sid_embed_bwd) -> (d_table [L * K, d], d_sep [d],
    d_prefix [prefix_rows, d]), None where not wanted or not part of the plan (has_sep; prefix_rows = 0: no prefix).
    d_x [B, T, d] float32; ids, mask, L, ld_item, prefix_idx: the forward's.  Each gradient is written whole, rows no
    token reads are zero, and a token whose index lies outside the table is dropped.  No atomics and no host read: the
    summation order depends on the shape and the ids alone, so the same inputs give the same bits on every run."""
    who = "sid_embed_bwd"
    L, K, prefix_rows = int(L), int(K), int(prefix_rows)
    if d_x.dtype != torch.float32 or d_x.dim() != 3:
        raise RqHipError(f"{who}: d_x must be a float32 [B, T, d] tensor, got {d_x.dtype} {tuple(d_x.shape)}")
    d = d_x.shape[2]
    if K < 1 or prefix_rows < 0:
        raise RqHipError(f"{who}: K={K}, prefix_rows={prefix_rows}")
    if not prefix_rows:
        prefix_idx = None
    ids, mask, elt, B, items, prefix_idx, ld_p = _sid_embed_plan(who, ids, mask, L, ld_item, d, prefix_idx)
    T = (prefix_rows > 0) + items * (L + bool(has_sep))
    if tuple(d_x.shape) != (B, T, d):
        raise RqHipError(f"{who}: d_x {tuple(d_x.shape)} does not match [{B}, {T}, {d}]")
    _need_gpu(d_x, ids)
    d_x = _aligned16(d_x.contiguous())
    need_sep, need_prefix = need_sep and bool(has_sep), need_prefix and prefix_rows > 0
    dev = d_x.device
    with torch.cuda.device(dev):
        make = torch.zeros if B == 0 else torch.empty      # without rows the sums are empty
        d_table = make((L * K, d), dtype=torch.float32, device=dev) if need_table else None
        d_sep = make((d,), dtype=torch.float32, device=dev) if need_sep else None
        d_prefix = make((prefix_rows, d), dtype=torch.float32, device=dev) if need_prefix else None
        nbytes = int(_lib.lib().rqhip_sid_embed_bwd_workspace_bytes(B, items, L, K, d))
        work = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev) if nbytes else None
        rc = _lib.lib().rqhip_sid_embed_bwd(_ptr(d_x), _ptr(ids), _ptr(mask), elt, B, items, L, int(ld_item), K, d,
                                            int(bool(has_sep)), int(prefix_rows > 0), _ptr(prefix_idx), ld_p, prefix_rows,
                                            _ptr(d_table), _ptr(d_sep), _ptr(d_prefix), _ptr(work), nbytes, _stream())
        check(rc, "rqhip_sid_embed_bwd")
    return d_table, d_sep, d_prefix


def seq_batch_supported(w: int, S: int) -> bool:
    """Whether seq_batch implements this shape (rqhip_seq_batch_supported): w in 2 .. 9 ids per item, S in 2 .. 256."""
    return bool(_lib.lib().rqhip_seq_batch_supported(int(w), int(S)))


def seq_batch(seq, rows: Tensor, table: Tensor, S: int, draws: Optional[Tensor] = None, token_types: bool = True):
    """A whole TokenizedSeqBatch in one launch (rqhip_seq_batch) from device-resident histories.
      seq: the CSR store of a data.processed.SeqData (its int64 tensors `offsets` [U + 1], `items` [nnz], `itemId_fut`
      [U], `userId` [U]); rows [B] int64 user indices, repeats allowed; table [n_items, w] int64, the tokenizer's
      cached ids; S the history length of a row.
      draws None: every row is its user's last min(S, n_hist) items with the stored future item as the target.
      draws [B, 2] int64 in [0, 2^62): row b is the window data.processed.seq_window(n_hist, *draws[b], S, True).
    Returns sem_ids [B, S * w] (-1 in padded slots), seq_mask [B, S * w] bool, sem_ids_fut [B, w], user_ids [B, 1] and,
    with token_types, the two token_type_ids tensors (else None) -- the fields, dtypes and bits of
    SemanticIdTokenizer.forward on the same windows.  An item id outside the table is padding, never an address.  No
    host read, no sync and no allocation whose size depends on data."""
    from data.schemas import TokenizedSeqBatch
    who = "seq_batch"
    tensors = {"offsets": seq.offsets, "items": seq.items, "itemId_fut": seq.itemId_fut, "userId": seq.userId, "rows": rows}
    for name, t in tensors.items():
        if t.dtype != torch.int64 or t.dim() != 1:
            raise RqHipError(f"{who}: {name} must be a 1-d int64 tensor, got {t.dtype} {tuple(t.shape)}")
    U, S = seq.userId.shape[0], int(S)
    if seq.offsets.shape[0] != U + 1 or seq.itemId_fut.shape[0] != U:
        raise RqHipError(f"{who}: offsets {tuple(seq.offsets.shape)} and itemId_fut {tuple(seq.itemId_fut.shape)} do not "
                         f"describe {U} users")
    if table.dtype != torch.int64 or table.dim() != 2:
        raise RqHipError(f"{who}: table must be an int64 [n_items, w] tensor, got {table.dtype} {tuple(table.shape)}")
    n_items, w = table.shape
    B = rows.shape[0]
    if draws is not None and (draws.dtype != torch.int64 or tuple(draws.shape) != (B, 2)):
        raise RqHipError(f"{who}: draws must be an int64 [{B}, 2] tensor, got {draws.dtype} {tuple(draws.shape)}")
    if not seq_batch_supported(w, S):
        raise RqHipError(f"{who}: (w, S) = ({w}, {S}) is not supported (w in 2 .. 9, S in 2 .. 256)")
    dev = _need_gpu(*tensors.values(), table, draws)
    offsets, items, fut, user, rows = (t.contiguous() for t in tensors.values())
    table = table.contiguous()
    draws = None if draws is None else draws.contiguous()
    with torch.cuda.device(dev):
        sem_ids = torch.empty((B, S * w), dtype=torch.int64, device=dev)
        seq_mask = torch.empty((B, S * w), dtype=torch.bool, device=dev)
        sem_ids_fut = torch.empty((B, w), dtype=torch.int64, device=dev)
        user_ids = torch.empty((B, 1), dtype=torch.int64, device=dev)
        tt = torch.empty((B, S * w), dtype=torch.int64, device=dev) if token_types else None
        tt_fut = torch.empty((B, w), dtype=torch.int64, device=dev) if token_types else None
        rc = _lib.lib().rqhip_seq_batch(_ptr(offsets), _ptr(items), _ptr(fut), _ptr(user), U, items.shape[0], _ptr(rows), B,
                                        _ptr(draws), _ptr(table), n_items, w, S, _ptr(sem_ids), _ptr(seq_mask),
                                        _ptr(sem_ids_fut), _ptr(user_ids), _ptr(tt), _ptr(tt_fut), _stream())
        check(rc, "rqhip_seq_batch")
    return TokenizedSeqBatch(user_ids=user_ids, sem_ids=sem_ids, sem_ids_fut=sem_ids_fut, seq_mask=seq_mask,
                             token_type_ids=tt, token_type_ids_fut=tt_fut)


def gumbel_matrix_path_min_rows(set_to: int = 0) -> int:
    """Query (set_to <= 0) or set the batch size from which the Gumbel level runs on the matrix instructions
    (rqhip_gumbel_matrix_path_min_rows); returns the previous value."""
    return int(_lib.lib().rqhip_gumbel_matrix_path_min_rows(int(set_to)))


def gumbel_forward(x: Tensor, codebook: Tensor, U: Tensor, temperature: float, beta: float):
    """One GUMBEL_SOFTMAX level, training (rqhip_gumbel_forward) -> (ids [B], emb [B,D], loss [B])."""
    _need_gpu(x, codebook, U)
    x, codebook, U = _f32c(x, "x"), _f32c(codebook, "codebook"), _f32c(U, "U")
    B, D = x.shape
    K = codebook.shape[0]
    if tuple(U.shape) != (B, K):
        raise RqHipError(f"U must be [B,K]=({B},{K}), got {tuple(U.shape)}")
    dev = x.device
    with torch.cuda.device(dev):
        ids = torch.empty((B,), dtype=torch.int64, device=dev)
        emb = torch.empty((B, D), dtype=torch.float32, device=dev)
        loss = torch.empty((B,), dtype=torch.float32, device=dev)
        rc = _lib.lib().rqhip_gumbel_forward(_ptr(x), B, D, _ptr(codebook), K, _ptr(U), temperature, beta, _ptr(ids),
                                             _ptr(emb), _ptr(loss), _stream())
        check(rc, "rqhip_gumbel_forward")
    return ids, emb, loss


def gumbel_backward(x: Tensor, codebook: Tensor, U: Tensor, temperature: float, beta: float, *,
                    g_emb: Optional[Tensor] = None, g_loss: Optional[Tensor] = None):
    """Backward of gumbel_forward (rqhip_gumbel_backward) -> (g_x [B,D], g_codebook [K,D])."""
    _need_gpu(x, codebook, U, g_emb, g_loss)
    x, codebook, U = _f32c(x, "x"), _f32c(codebook, "codebook"), _f32c(U, "U")
    g_emb, g_loss = _f32c(g_emb, "g_emb"), _f32c(g_loss, "g_loss")
    B, D = x.shape
    K = codebook.shape[0]
    dev = x.device
    with torch.cuda.device(dev):
        l = _lib.lib()
        g_x = torch.empty((B, D), dtype=torch.float32, device=dev)
        g_cb = torch.empty((K, D), dtype=torch.float32, device=dev)
        wsb = l.rqhip_gumbel_backward_workspace_bytes(B, D, K)
        ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
        rc = l.rqhip_gumbel_backward(_ptr(x), B, D, _ptr(codebook), K, _ptr(U), temperature, beta, _ptr(g_emb),
                                     _ptr(g_loss), _ptr(g_x), _ptr(g_cb), _ptr(ws), wsb, _stream())
        check(rc, "rqhip_gumbel_backward")
    return g_x, g_cb


def profile_enable(max_records: int) -> None:
    """Bench-only: time the main rq_forward kernel of every following call with HIP events on its stream."""
    check(_lib.lib().rqhip_profile_enable(int(max_records)), "rqhip_profile_enable")


def profile_read(cap: int = 4096):
    """Durations (ms) of the rq_forward kernels recorded since the last read (synchronises them)."""
    import ctypes as C
    buf = (C.c_float * cap)()
    n = C.c_int(0)
    check(_lib.lib().rqhip_profile_read(buf, cap, C.byref(n)), "rqhip_profile_read")
    return [buf[i] for i in range(n.value)]


def profile_select(*kinds: str) -> None:
    """Record only launches of these kinds (names of _lib.PROF_TAGS); no argument = every kind."""
    mask = 0
    for k in kinds:
        if k == "none":          # record nothing until the next select
            check(_lib.lib().rqhip_profile_select(0), "rqhip_profile_select")
            return
        mask |= 1 << next(t for t, n in _lib.PROF_TAGS.items() if n == k)
    check(_lib.lib().rqhip_profile_select(mask if kinds else 0xFFFFFFFF), "rqhip_profile_select")


def profile_read_tagged(cap: int = 65536):
    """Every record since the last read as (kind, ms, algorithmic flops, algorithmic bytes); kinds: _lib.PROF_TAGS."""
    import ctypes as C
    buf = (_lib.ProfileRecord * cap)()
    n = C.c_int(0)
    check(_lib.lib().rqhip_profile_read_tagged(buf, cap, C.byref(n)), "rqhip_profile_read_tagged")
    return [(_lib.PROF_TAGS.get(buf[i].tag, str(buf[i].tag)), buf[i].ms, buf[i].flops, buf[i].bytes) for i in range(n.value)]


def _rows(t: Tensor, name: str) -> Tensor:
    """[B,N] fp32 with unit column stride (row stride may exceed N: slices of a wider matrix are fine)."""
    if t.dtype != torch.float32 or t.dim() != 2:
        raise RqHipError(f"{name} must be a 2-D float32 tensor")
    return t if t.stride(1) == 1 and t.stride(0) >= t.shape[1] else t.contiguous()


def recon_loss_forward(x_hat: Tensor, x: Tensor) -> Tensor:
    """out[b] = sum_d (x_hat - x)^2 (rqhip_recon_loss_forward; reference modules/loss.py:5-10)."""
    _need_gpu(x_hat, x)
    x_hat, x = _rows(x_hat, "x_hat"), _rows(x, "x")
    if x_hat.shape != x.shape:
        raise RqHipError(f"shape mismatch {tuple(x_hat.shape)} vs {tuple(x.shape)}")
    B, N = x.shape
    with torch.cuda.device(x.device):
        out = torch.empty((B,), dtype=torch.float32, device=x.device)
        rc = _lib.lib().rqhip_recon_loss_forward(_ptr(x_hat), x_hat.stride(0), _ptr(x), x.stride(0), B, N, _ptr(out),
                                                 _stream())
        check(rc, "rqhip_recon_loss_forward")
    return out


def recon_loss_backward(x_hat: Tensor, x: Tensor, g_out: Tensor, need_hat: bool = True, need_x: bool = False):
    _need_gpu(x_hat, x, g_out)
    x_hat, x, g_out = _rows(x_hat, "x_hat"), _rows(x, "x"), _f32c(g_out, "g_out")
    B, N = x.shape
    with torch.cuda.device(x.device):
        g_hat = torch.empty((B, N), dtype=torch.float32, device=x.device) if need_hat else None
        g_x = torch.empty((B, N), dtype=torch.float32, device=x.device) if need_x else None
        rc = _lib.lib().rqhip_recon_loss_backward(_ptr(x_hat), x_hat.stride(0), _ptr(x), x.stride(0), _ptr(g_out), B, N,
                                                  _ptr(g_hat), _ptr(g_x), _stream())
        check(rc, "rqhip_recon_loss_backward")
    return g_hat, g_x


def recon_spec_ok(x_hat: Tensor, x: Tensor) -> bool:
    """Can the speculative reconstruction-loss pair take these tensors (float4 layout)?"""
    return (x_hat.dim() == 2 and x_hat.shape == x.shape and x_hat.shape[1] % 4 == 0 and x_hat.stride(1) == 1
            and x.stride(1) == 1 and x_hat.stride(0) % 4 == 0 and x.stride(0) % 4 == 0
            and x_hat.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0 and x_hat.dtype == torch.float32
            and x.dtype == torch.float32)


def recon_loss_forward_spec(x_hat: Tensor, x: Tensor, row_scale: float):
    """out[b] = sum_d (x_hat - x)^2 and the expected gradient g_spec = 2 (x_hat - x) * row_scale in one pass
    (rqhip_recon_loss_forward_spec).  Returns (out [B], g_spec [B,N])."""
    _need_gpu(x_hat, x)
    B, N = x.shape
    with torch.cuda.device(x.device):
        out = torch.empty((B,), dtype=torch.float32, device=x.device)
        g_spec = torch.empty((B, N), dtype=torch.float32, device=x.device)
        rc = _lib.lib().rqhip_recon_loss_forward_spec(_ptr(x_hat), x_hat.stride(0), _ptr(x), x.stride(0), B, N,
                                                      row_scale, _ptr(out), _ptr(g_spec), _stream())
        check(rc, "rqhip_recon_loss_forward_spec")
    return out, g_spec


def recon_loss_backward_spec(x_hat: Tensor, x: Tensor, g_out: Tensor, row_scale: float, g_spec: Tensor) -> Tensor:
    """Fix up g_spec in place for rows whose upstream gradient differs from row_scale; returns g_spec."""
    _need_gpu(x_hat, x, g_out, g_spec)
    g_out = _f32c(g_out, "g_out")
    B, N = x.shape
    with torch.cuda.device(x.device):
        rc = _lib.lib().rqhip_recon_loss_backward_spec(_ptr(x_hat), x_hat.stride(0), _ptr(x), x.stride(0), _ptr(g_out),
                                                       B, N, row_scale, _ptr(g_spec), _stream())
        check(rc, "rqhip_recon_loss_backward_spec")
    return g_spec


def loss_means_backward(g_loss: Optional[Tensor], g_recon: Optional[Tensor], g_quant: Optional[Tensor], n: int,
                        want_recon: bool = True, want_quant: bool = True):
    """Row gradients of the three means (rqhip_loss_means_backward): two dense [n] vectors (None where not wanted)."""
    ref = next((g for g in (g_loss, g_recon, g_quant) if g is not None), None)
    if ref is None or not (want_recon or want_quant):
        return None, None
    _need_gpu(ref)
    gs = [None if g is None else _f32c(g.reshape(()), "g") for g in (g_loss, g_recon, g_quant)]
    with torch.cuda.device(ref.device):
        rows_r = torch.empty((n,), dtype=torch.float32, device=ref.device) if want_recon else None
        rows_q = torch.empty((n,), dtype=torch.float32, device=ref.device) if want_quant else None
        check(_lib.lib().rqhip_loss_means_backward(_ptr(gs[0]), _ptr(gs[1]), _ptr(gs[2]), n, _ptr(rows_r), _ptr(rows_q),
                                                   _stream()), "rqhip_loss_means_backward")
    return rows_r, rows_q


def loss_means(recon: Tensor, quant: Tensor) -> Tensor:
    """[3] = mean(recon + quant), mean(recon), mean(quant) in one launch (rqhip_loss_means)."""
    _need_gpu(recon, quant)
    recon, quant = _f32c(recon, "recon"), _f32c(quant, "quant")
    if recon.dim() != 1 or recon.shape != quant.shape or recon.numel() == 0:
        raise RqHipError(f"loss_means: need two non-empty [B] tensors, got {tuple(recon.shape)}, {tuple(quant.shape)}")
    with torch.cuda.device(recon.device):
        out = torch.empty((3,), dtype=torch.float32, device=recon.device)
        l = _lib.lib()
        from . import linear as _lin_mod
        key = (recon.device.index, _stream())
        # (the meeting place must have been zeroed by an EXECUTED fill: a first use under hipGraph capture takes the one-workgroup kernel)
        fresh_in_capture = key not in _LOSS_MEANS_WS and torch.cuda.is_current_stream_capturing()
        if recon.numel() <= 4096 or not _lin_mod.trims_on() or fresh_in_capture:        # one workgroup's worth: the single-workgroup kernel
            check(l.rqhip_loss_means(_ptr(recon), _ptr(quant), recon.numel(), _ptr(out), _stream()), "rqhip_loss_means")
        else:                            # many workgroups; their meeting place is zeroed once per (device, stream) and re-armed by the kernel
            ws = _LOSS_MEANS_WS.get(key)
            if ws is None:
                ws = _LOSS_MEANS_WS[key] = torch.zeros((l.rqhip_loss_means_workspace_bytes(),), dtype=torch.uint8, device=recon.device)
            check(l.rqhip_loss_means_ws(_ptr(recon), _ptr(quant), recon.numel(), _ptr(out), _ptr(ws), ws.numel(), _stream()),
                  "rqhip_loss_means_ws")
    return out


_LOSS_MEANS_WS = {}


def linear_wgrad_supported(n_out: int, n_in: int) -> bool:
    return bool(_lib.lib().rqhip_linear_wgrad_supported(int(n_out), int(n_in)))


def linear_wgrad(g: Tensor, y: Optional[Tensor], x: Tensor, *, want_masked: bool = True, out: Optional[Tensor] = None,
                 exact_fp32: bool = False, g_col_max: Optional[Tensor] = None, x_col_max: Optional[Tensor] = None):
    """dW [N,K] = (g * (y > 0))^T x with the ReLU backward fused (rqhip_linear_wgrad*); y None = layer without ReLU.
    Returns (dW, g_pre): g_pre = the masked gradient in a fresh tensor when `want_masked` and y is given (the input
    of the data-gradient GEMM that follows), g itself when there is no mask, None when not wanted.  `out`: a
    contiguous fp32 [N,K] tensor to receive dW (e.g. the parameter's slice of a flat gradient buffer).
    g_col_max / x_col_max (int32 [N] / [K], `maxima`): the two-piece fp16 arithmetic under exact column scales
    (rqhip_linear_wgrad_f16, the product path); without them the three-piece bf16 kernel of round 3.
    exact_fp32: force the fp32-MFMA kernel with the oracle-restated summation order (RQHIP_WGRAD_FP32)."""
    _need_gpu(g, y, x, g_col_max, x_col_max)
    g, x = _f32c(g, "g"), _f32c(x, "x")
    y = _f32c(y, "y")
    if g.dim() != 2 or x.dim() != 2 or g.shape[0] != x.shape[0] or (y is not None and y.shape != g.shape):
        raise RqHipError(f"linear_wgrad: shapes g {tuple(g.shape)}, x {tuple(x.shape)}")
    M, N = g.shape
    K = x.shape[1]
    f16 = g_col_max is not None or x_col_max is not None
    if f16 and (exact_fp32 or g_col_max is None or x_col_max is None or g_col_max.numel() != N or x_col_max.numel() != K
                or g_col_max.dtype != torch.int32 or x_col_max.dtype != torch.int32):
        raise RqHipError("linear_wgrad: the fp16 path needs BOTH column-maxima vectors (int32 [N] and [K]) and no exact_fp32")
    dev = g.device
    with torch.cuda.device(dev):
        l = _lib.lib()
        if out is not None and (tuple(out.shape) != (N, K) or out.dtype != torch.float32 or not out.is_contiguous()):
            raise RqHipError("linear_wgrad: `out` must be a contiguous float32 [N,K] tensor")
        dw = out if out is not None else torch.empty((N, K), dtype=torch.float32, device=dev)
        wsb = l.rqhip_linear_wgrad_workspace_bytes(M, N, K)
        ws = torch.empty((max(wsb, 16),), dtype=torch.uint8, device=dev)
        gm = torch.empty_like(g) if (want_masked and y is not None) else None
        if f16:
            rc = l.rqhip_linear_wgrad_f16(_ptr(g), _ptr(y), _ptr(x), M, N, K, _ptr(g_col_max), _ptr(x_col_max), _ptr(gm),
                                          _ptr(dw), _ptr(ws), wsb, _stream())
            check(rc, "rqhip_linear_wgrad_f16")
        else:
            rc = l.rqhip_linear_wgrad_ex(_ptr(g), _ptr(y), _ptr(x), M, N, K, _ptr(gm), _ptr(dw), _ptr(ws), wsb,
                                         _lib.WGRAD_FP32 if exact_fp32 else 0, _stream())
            check(rc, "rqhip_linear_wgrad_ex")
    return dw, (g if y is None else gm)


def linear_wgrad_f16_batch_ranges(M: int, shapes) -> int:
    """The common number of row ranges rqhip_linear_wgrad_f16_batch would cut `shapes` = [(N, K), ...] into over M rows; 0 = not batchable
    (2..4 layers, every dW tiled 256 x 256, more than 128 rows)."""
    n = len(shapes)
    if n < 2 or n > 4:
        return 0
    ci = C.c_int * n
    return int(_lib.lib().rqhip_linear_wgrad_f16_batch_plan(int(M), ci(*[int(a) for a, _ in shapes]), ci(*[int(b) for _, b in shapes]), n))


def linear_wgrad_f16_batch(jobs, outs=None):
    """The weight gradients of 2..4 layers in ONE launch (rqhip_linear_wgrad_f16_batch): `jobs` = [(g [M, N_j] already masked by the layer's
    ReLU, x [M, K_j], g_col_max int32 [N_j], x_col_max int32 [K_j]), ...], every dW tiled 256 x 256; `outs[j]`: a contiguous fp32
    [N_j, K_j] tensor to receive dW_j (or None).  Returns [dW_j]."""
    n = len(jobs)
    gs = [_f32c(j[0], "g") for j in jobs]
    xs = [_f32c(j[1], "x") for j in jobs]
    _need_gpu(*gs, *xs, *[j[2] for j in jobs], *[j[3] for j in jobs])
    M, dev = gs[0].shape[0], gs[0].device
    shapes = [(g.shape[1], x.shape[1]) for g, x in zip(gs, xs)]
    for i, (g, x, gm, xm) in enumerate(zip(gs, xs, [j[2] for j in jobs], [j[3] for j in jobs])):
        if (g.dim() != 2 or x.dim() != 2 or g.shape[0] != M or x.shape[0] != M or gm.dtype != torch.int32 or xm.dtype != torch.int32
                or gm.numel() != g.shape[1] or xm.numel() != x.shape[1] or not gm.is_contiguous() or not xm.is_contiguous()):
            raise RqHipError(f"linear_wgrad_f16_batch: job {i}: g {tuple(g.shape)}, x {tuple(x.shape)}, maxima int32 [N] / [K]; one M")
    if linear_wgrad_f16_batch_ranges(M, shapes) < 1:
        raise RqHipError(f"linear_wgrad_f16_batch: {shapes} over {M} rows is not batchable (linear_wgrad_f16_batch_ranges)")
    with torch.cuda.device(dev):
        l = _lib.lib()
        dws = []
        for i, (N, K) in enumerate(shapes):
            out = outs[i] if outs is not None else None
            if out is not None and (tuple(out.shape) != (N, K) or out.dtype != torch.float32 or not out.is_contiguous()):
                raise RqHipError("linear_wgrad_f16_batch: `outs[j]` must be a contiguous float32 [N, K] tensor")
            dws.append(out if out is not None else torch.empty((N, K), dtype=torch.float32, device=dev))
        ci = C.c_int * n
        Ns, Ks = ci(*[a for a, _ in shapes]), ci(*[b for _, b in shapes])
        wsb = l.rqhip_linear_wgrad_f16_batch_workspace_bytes(M, Ns, Ks, n)
        ws = torch.empty((max(wsb, 16),), dtype=torch.uint8, device=dev)
        arr = (_lib.WgradJob * n)()
        for i in range(n):
            arr[i].g, arr[i].x, arr[i].N, arr[i].K = gs[i].data_ptr(), xs[i].data_ptr(), shapes[i][0], shapes[i][1]
            arr[i].g_col_max, arr[i].x_col_max, arr[i].dW = jobs[i][2].data_ptr(), jobs[i][3].data_ptr(), dws[i].data_ptr()
        check(l.rqhip_linear_wgrad_f16_batch(arr, n, M, _ptr(ws), wsb, _stream()), "rqhip_linear_wgrad_f16_batch")
    return dws


def linear_wgrad_jobs_supported(n_out: int, n_in: int) -> bool:
    return bool(_lib.lib().rqhip_linear_wgrad_jobs_supported(int(n_out), int(n_in)))


WGRAD_JOBS_MAX = 8


def linear_wgrad_jobs(jobs, outs=None):
    """The weight gradients of several layers in ONE launch (rqhip_linear_wgrad_jobs, csrc/wgrad_jobs.hip): `jobs` =
    [(g [M, N_i] ALREADY masked by the layer's ReLU, x [M, K_i]), ...], at most 8, one M; `outs[i]`: a contiguous fp32
    [N_i, K_i] tensor to receive dW_i (or None).  Returns [dW_i].  The small-batch path of the MLP stacks."""
    if not jobs:
        return []
    if len(jobs) > WGRAD_JOBS_MAX:
        raise RqHipError(f"linear_wgrad_jobs: at most {WGRAD_JOBS_MAX} jobs per launch (got {len(jobs)})")
    gs = [_f32c(g, "g") for g, _ in jobs]
    xs = [_f32c(x, "x") for _, x in jobs]
    _need_gpu(*gs, *xs)
    M, dev = gs[0].shape[0], gs[0].device
    dws = []
    for i, (g, x) in enumerate(zip(gs, xs)):
        if g.dim() != 2 or x.dim() != 2 or g.shape[0] != M or x.shape[0] != M or g.device != dev or x.device != dev:
            raise RqHipError(f"linear_wgrad_jobs: job {i}: g {tuple(g.shape)}, x {tuple(x.shape)}; every job has M = {M} rows")
        N, K = g.shape[1], x.shape[1]
        out = outs[i] if outs is not None else None
        if out is not None and (tuple(out.shape) != (N, K) or out.dtype != torch.float32 or not out.is_contiguous()):
            raise RqHipError("linear_wgrad_jobs: `outs[i]` must be a contiguous float32 [N,K] tensor")
        dws.append(out if out is not None else torch.empty((N, K), dtype=torch.float32, device=dev))
    if M == 0:          # no rows: every gradient is zero (and an empty tensor has no address to hand over)
        for d in dws:
            d.zero_()
        return dws
    n = len(jobs)
    vp, ci = C.c_void_p * n, C.c_int * n
    with torch.cuda.device(dev):
        rc = _lib.lib().rqhip_linear_wgrad_jobs(vp(*[_ptr(g) for g in gs]), vp(*[_ptr(x) for x in xs]), vp(*[_ptr(d) for d in dws]),
                                                ci(*[g.shape[1] for g in gs]), ci(*[x.shape[1] for x in xs]), n, M, _stream())
        check(rc, "rqhip_linear_wgrad_jobs")
    return dws


def gemm_split_supported(n_cols: int, n_red: int) -> bool:
    return bool(_lib.lib().rqhip_gemm_split_supported(int(n_cols), int(n_red)))


F16X2, BF16X3 = _lib.SPLIT_F16X2, _lib.SPLIT_BF16X3


def weight_images(jobs, arith: int = F16X2):
    """The split-GEMM images of several weight matrices in ONE launch (rqhip_weight_images): `jobs` = [(w, transpose), ...];
    of w [rows, cols] itself (forward: C = A w^T) or of w^T (`transpose`: data gradient, C = A w).  Returns one opaque
    uint8 tensor per job (views of a single allocation)."""
    if not jobs:
        return []
    ws = [_f32c(w.detach(), "w") for w, _ in jobs]
    dev = _need_gpu(*ws)
    l = _lib.lib()
    sizes = []
    for w, (_, tr) in zip(ws, jobs):
        rows, cols = w.shape
        Nc, R = (cols, rows) if tr else (rows, cols)
        nb = l.rqhip_weight_image_bytes(Nc, R, int(arith))
        if nb == 0:
            raise RqHipError(f"weight_images: unsupported shape {tuple(w.shape)} (transpose={bool(tr)})")
        sizes.append(nb)
    with torch.cuda.device(dev):
        slots = [(nb + 255) // 256 * 256 for nb in sizes]          # every image 256-byte aligned inside the arena
        arena = torch.empty((sum(slots),), dtype=torch.uint8, device=dev)
        arr = (_lib.ImageJob * len(jobs))()
        images, off = [], 0
        for i, (w, (_, tr), nb, slot) in enumerate(zip(ws, jobs, sizes, slots)):
            img = arena[off:off + nb]                               # exactly the image: no uninitialised padding in the view
            off += slot
            arr[i].w, arr[i].rows, arr[i].cols = w.data_ptr(), w.shape[0], w.shape[1]
            arr[i].transpose, arr[i].arith = int(bool(tr)), int(arith)
            arr[i].image, arr[i].image_bytes = img.data_ptr(), nb
            images.append(img)
        check(l.rqhip_weight_images(arr, len(jobs), _stream()), "rqhip_weight_images")
    return images


def weight_planes(w: Tensor, transpose: bool = False, arith: int = BF16X3) -> Tensor:
    """One image (`weight_images` with a single job; round 3's name and default arithmetic)."""
    return weight_images([(w, transpose)], arith)[0]


def maxima(a: Tensor, y: Optional[Tensor] = None, *, rows: bool = True, cols: bool = True, write_masked: bool = False):
    """(row_max [1, M] or None, col_max [R] or None, masked or None): int32 tensors holding the bit patterns of the largest
    |value| of every row / column of a [M, R] (rqhip_maxima) -- the exact power-of-two scales of the fp16 split kernels are
    derived from them.  With y: of `a` masked by y > 0 (the ReLU backward), returned as `masked` when `write_masked`."""
    _need_gpu(a, y)
    a, y = _f32c(a, "a"), _f32c(y, "y")
    M, R = a.shape
    if y is not None and y.shape != a.shape:
        raise RqHipError(f"maxima: y is {tuple(y.shape)}, expected {tuple(a.shape)}")
    with torch.cuda.device(a.device):
        rm = torch.empty((1, M), dtype=torch.int32, device=a.device) if rows else None
        cm = torch.zeros((R,), dtype=torch.int32, device=a.device) if cols else None
        out = torch.empty_like(a) if (write_masked and y is not None) else None
        check(_lib.lib().rqhip_maxima(_ptr(a), _ptr(y), _ptr(out), M, R, _ptr(rm), _ptr(cm), _stream()), "rqhip_maxima")
    return rm, cm, out


def gemm_split_ex(a: Tensor, image: Tensor, n_cols: int, *, arith: int = F16X2, epilogue: int = _lib.EPI_STORE,
                  aux: Optional[Tensor] = None, row_scale: float = 0.0, a_row_max: Optional[Tensor] = None,
                  want_row_max: bool = False, col_max_out: Optional[Tensor] = None, tile_rows: int = 0):
    """C [M, n_cols] = epilogue(a [M, R] . image^T) (rqhip_gemm_split_ex).  Returns (C, loss_rows or None, c_row_max or None):
    loss_rows for EPI_RECON; c_row_max [column tiles, M] int32 when `want_row_max`; `col_max_out` (int32 [n_cols], ZEROED by
    the caller, or a slice of a zeroed arena) receives the column maxima of C.  arith F16X2 needs `a_row_max` [parts, M]."""
    _need_gpu(a, image, aux, a_row_max, col_max_out)
    a, aux = _f32c(a, "a"), _f32c(aux, "aux")
    M, R = a.shape
    if aux is not None and tuple(aux.shape) != (M, n_cols):
        raise RqHipError(f"gemm_split: aux is {tuple(aux.shape)}, expected {(M, n_cols)}")
    if a_row_max is not None and (a_row_max.dtype != torch.int32 or a_row_max.dim() != 2 or a_row_max.shape[1] != M
                                  or not a_row_max.is_contiguous()):
        raise RqHipError("gemm_split: a_row_max must be a contiguous int32 [parts, M] tensor")
    if col_max_out is not None and (col_max_out.dtype != torch.int32 or col_max_out.numel() != n_cols
                                    or not col_max_out.is_contiguous()):
        raise RqHipError("gemm_split: col_max_out must be a contiguous int32 [n_cols] tensor")
    with torch.cuda.device(a.device):
        l = _lib.lib()
        c = torch.empty((M, n_cols), dtype=torch.float32, device=a.device)
        args = _lib.GemmArgs()
        args.A, args.M, args.R, args.image, args.Nc = a.data_ptr(), M, R, image.data_ptr(), int(n_cols)
        args.arith, args.epilogue, args.tile_rows, args.C = int(arith), int(epilogue), int(tile_rows), c.data_ptr()
        args.aux, args.row_scale = _ptr(aux), float(row_scale)
        rows = ws = None
        if epilogue == _lib.EPI_RECON:
            rows = torch.empty((M,), dtype=torch.float32, device=a.device)
            nbytes = l.rqhip_gemm_split_recon_workspace_bytes(M, int(n_cols))
            ws = torch.empty((max(nbytes, 4),), dtype=torch.uint8, device=a.device)
            args.loss_rows, args.workspace, args.workspace_bytes = rows.data_ptr(), ws.data_ptr(), nbytes
        if a_row_max is not None:
            args.a_row_max, args.a_row_parts = a_row_max.data_ptr(), a_row_max.shape[0]
        crm = torch.empty((n_cols // (256 if n_cols % 256 == 0 else 128), M), dtype=torch.int32, device=a.device) if want_row_max else None
        args.c_row_max, args.c_col_max = _ptr(crm), _ptr(col_max_out)
        import ctypes as C
        check(l.rqhip_gemm_split_ex(C.byref(args), _stream()), "rqhip_gemm_split_ex")
    return c, rows, crm


def gemm_split(a: Tensor, planes: Tensor, n_cols: int, relu: bool = False, tile_rows: int = 0, arith: int = BF16X3) -> Tensor:
    """C [M, n_cols] = a [M, R] . image^T with the optional ReLU epilogue.  arith BF16X3 (default here: round 3's call) or
    F16X2, for which the row maxima of `a` are computed by a `maxima` pass first (callers that chain layers use
    `gemm_split_ex` and hand the maxima over instead)."""
    rm = maxima(a, cols=False)[0] if arith == F16X2 else None
    return gemm_split_ex(a, planes, n_cols, arith=arith, epilogue=_lib.EPI_RELU if relu else _lib.EPI_STORE, a_row_max=rm,
                         tile_rows=tile_rows)[0]


def gemm_split_recon(a: Tensor, planes: Tensor, n_cols: int, x: Tensor, row_scale: float, arith: int = BF16X3):
    """The last decoder layer fused with the reconstruction loss (RQHIP_EPI_RECON): with x_hat = a . image^T (never stored)
    returns (g, loss_rows): g [M, n_cols] = (2 (x_hat - x)) * row_scale and loss_rows [M] = sum (x_hat - x)^2."""
    if tuple(x.shape) != (a.shape[0], n_cols):
        raise RqHipError(f"gemm_split_recon: x is {tuple(x.shape)}, expected {(a.shape[0], n_cols)}")
    rm = maxima(a, cols=False)[0] if arith == F16X2 else None
    g, rows, _ = gemm_split_ex(a, planes, n_cols, arith=arith, epilogue=_lib.EPI_RECON, aux=x, row_scale=row_scale, a_row_max=rm)
    return g, rows


def recon_rescale_rows(g_spec: Tensor, g_out: Tensor, row_scale: float, row_max: Optional[Tensor] = None,
                       col_max: Optional[Tensor] = None) -> Tensor:
    """In place: rows of g_spec whose upstream gradient g_out[row] is not row_scale (bit compare) are multiplied by
    g_out[row] / row_scale (rqhip_recon_rescale_rows_ex); returns g_spec.  row_max [parts, B] / col_max [N] (int32, the
    maxima the fused epilogue emitted for g_spec) are brought up to date for the rows that change."""
    _need_gpu(g_spec, g_out, row_max, col_max)
    g_out = _f32c(g_out, "g_out")
    B, N = g_spec.shape
    with torch.cuda.device(g_spec.device):
        check(_lib.lib().rqhip_recon_rescale_rows_ex(_ptr(g_out), B, N, float(row_scale), _ptr(g_spec), _ptr(row_max),
                                                     0 if row_max is None else row_max.shape[0], _ptr(col_max), _stream()),
              "rqhip_recon_rescale_rows_ex")
    return g_spec
