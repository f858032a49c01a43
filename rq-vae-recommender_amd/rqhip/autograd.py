"""torch.autograd bridges: forward and backward both run in HIP through the C ABI.

These Functions are the seam between the reference-shaped Python modules (modules/quantize.py,
modules/rqvae.py) and librqhip.so.  They hold no arithmetic of their own.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from . import ops


def _dense(g: Optional[Tensor]) -> Optional[Tensor]:
    """Upstream gradients may arrive as None, expanded views or non-contiguous tensors."""
    if g is None:
        return None
    return g.contiguous()


class RqStackFunction(torch.autograd.Function):
    """L chained quantisation levels (EVAL / STE / ROTATION) as one differentiable op.

    forward(res0 [B,D], codebooks [L,K,D], mode, beta, want_levels) ->
        embs [L,B,D], residuals [L,B,D], ids [L,B], loss [B], emb_sum [B,D], embs_norm [B,L]
    (embs / residuals are empty tensors when want_levels is False: the fused training step only consumes
    emb_sum, loss and embs_norm, see modules/rqvae.py.)
    """

    @staticmethod
    def forward(ctx, res0: Tensor, codebooks: Tensor, mode: int, beta: float, want_levels: bool, grad_sink=None):
        """grad_sink (optional): object with `.view` ([L,K,D] slice of a flat gradient buffer) and `.params` (the L
        codebook parameters); the codebook gradient is written there when it is the first gradient of the step."""
        out = ops.rq_forward(res0, codebooks, mode, beta, want_embs=want_levels, want_residuals=want_levels)
        ctx.set_materialize_grads(False)   # outputs nobody used arrive as None (= NULL at the C ABI), not as zero tensors
        ctx.save_for_backward(res0, codebooks, out.ids)
        ctx.mode, ctx.beta, ctx.want_levels, ctx.grad_sink = mode, beta, want_levels, grad_sink
        embs = out.embs if want_levels else res0.new_empty((0,))
        residuals = out.residuals if want_levels else res0.new_empty((0,))
        if want_levels:
            ctx.mark_non_differentiable(out.ids, out.embs_norm)
        else:  # one call: a second mark_non_differentiable would replace the first
            ctx.mark_non_differentiable(out.ids, out.embs_norm, embs, residuals)
        return embs, residuals, out.ids, out.loss, out.emb_sum, out.embs_norm

    @staticmethod
    def backward(ctx, g_embs, g_resid, _g_ids, g_loss, g_embsum, _g_norm):
        res0, codebooks, ids = ctx.saved_tensors
        need_res0, need_cb = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_res0 or need_cb):
            return None, None, None, None, None, None
        if not ctx.want_levels:
            g_embs = g_resid = None
        sink = ctx.grad_sink
        out_cb = None
        if need_cb and sink is not None and tuple(sink.view.shape) == tuple(codebooks.shape) and all(
                p.grad is None and getattr(p, "_rq_sink_epoch", -1) != sink.owner.epoch for p in sink.params):
            out_cb = sink.view      # first gradient of the step: straight into the flat buffer (autograd's stack backward
                                    # hands each level's slice to its parameter as a view); claimed for this epoch, so a
                                    # second pass of the same model under one loss accumulates through autograd instead
            for p in sink.params:
                p._rq_sink_epoch = sink.owner.epoch
        g_res0, g_cb = ops.rq_backward(res0, codebooks, ctx.mode, ctx.beta, ids, g_embs=_dense(g_embs),
                                       g_embsum=_dense(g_embsum), g_resid=_dense(g_resid), g_loss=_dense(g_loss),
                                       need_res0=need_res0, need_codebooks=need_cb, out_g_codebooks=out_cb,
                                       cbgrad=ops.cbgrad_default())
        return g_res0, (g_cb.view_as(g_cb) if out_cb is not None else g_cb), None, None, None, None


class RqSeamFunction(torch.autograd.Function):
    """The RQ <-> MLP seam as ONE differentiable op and ONE forward launch (rqhip_rq_seam; reference modules/rqvae.py:118-139,146 with the
    last encoder Linear of modules/encoder.py:25-38 in front and the first decoder Linear + ReLU behind):

        forward(h [B,128], w_in [32,128], codebooks [L,K,32], w_out [128,32], mode, beta, grad_sink, want_scales)
            -> ids [L,B], loss [B], embs_norm [B,L], d [B,128] = relu((sum of the levels' outputs) w_out^T),
               row maxima [4,B] and column maxima [128] of d (int32 bit patterns; empty without want_scales)

    res0 = h w_in^T and the sum of the levels' outputs stay inside (saved for the backward).  Backward, composed of the same kernels:
    the decoder-side data gradient with the ReLU backward applied on load, the quantiser's closed-form backward (csrc/rq_backward.hip),
    the encoder-side data gradient with the ReLU backward of the layer below and its maxima in the epilogue (handed to the encoder
    stack's node: rqhip/linear.py:handoff_grad), and the two 32-wide weight gradients.  Same bits as running the three pieces as separate
    launches (tests/test_gpu_seam.py), which is what every other path through these layers does (rqhip/linear.py:chain_*)."""

    @staticmethod
    def forward(ctx, h: Tensor, w_in: Tensor, codebooks: Tensor, w_out: Tensor, mode: int, beta: float, grad_sink, want_scales: bool):
        from . import _lib
        from . import linear as _lin
        # (one zeroed buffer for the column maxima of this launch's output and of the backward's: one fill launch, not two)
        both = _lin.zeros_i32(2 * ops.SEAM_H, h.device) if want_scales else None
        cols = both[:ops.SEAM_H] if want_scales else None
        ctx.bwd_cols = both[ops.SEAM_H:] if (want_scales and torch.is_grad_enabled()) else None
        r = ops.rq_seam(h=h, w_in=w_in.detach(), codebooks=codebooks.detach(), mode=mode, beta=beta, w_out=w_out.detach(),
                        epilogue=_lib.EPI_RELU, want_row_max=want_scales, col_max_out=cols)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(h, w_in, codebooks, w_out, r.res0, r.ids, r.emb_sum, r.out)
        ctx.mode, ctx.beta, ctx.grad_sink, ctx.want_scales = mode, beta, grad_sink, want_scales
        # the maxima of d the decoder's split kernels scale by travel as two more (non-differentiable) outputs; empty when not wanted
        rmax = r.out_row_max if want_scales else h.new_empty((0,), dtype=torch.int32)
        cmax = cols if want_scales else h.new_empty((0,), dtype=torch.int32)
        ctx.mark_non_differentiable(r.ids, r.embs_norm, rmax, cmax)
        return r.ids, r.loss, r.embs_norm, r.out, rmax, cmax

    @staticmethod
    def backward(ctx, _g_ids, g_loss, _g_norm, g_d, _g_rmax=None, _g_cmax=None):
        from . import linear as _lin
        from .dist import claim_grad_sink
        h, w_in, codebooks, w_out, res0, ids, emb_sum, d = ctx.saved_tensors
        need_h, need_win, need_cb, need_wout = ctx.needs_input_grad[:4]
        g_d, g_loss = _dense(g_d), _dense(g_loss)
        B = h.shape[0]
        jobs = _lin.wgrad_jobs_ok(B, [tuple(w_out.shape), tuple(w_in.shape)])     # small batches: both weight gradients in ONE launch, at the end
        pending = []
        gw_out = gw_in = None
        # 1. decoder side: d = relu(s w_out^T)
        g_es = None
        if g_d is not None:
            g_dm = None
            if need_wout:
                if jobs:
                    g_dm = torch.ops.aten.threshold_backward(g_d, d, 0.0)     # (the job-table kernel takes the masked gradient as a tensor)
                    pending.append(_lin.WgradJob(w_out, g_dm, emb_sum, None, None, claim_grad_sink(w_out)))
                else:
                    sink = claim_grad_sink(w_out)
                    gw, gp, _ = _lin.weight_grad(g_d, d, emb_sum, w_out, out=sink, want_masked=False)
                    gw_out = gw.view_as(gw) if sink is not None else gw
                    g_dm = gp if (gp is not None and gp is not g_d) else None
            if need_h or need_win or need_cb:
                g_es = (_lin.chain_input_grad(g_dm, w_out)[0] if g_dm is not None
                        else _lin.chain_input_grad(g_d, w_out, g_mask=d)[0])       # the ReLU backward on load
        # 2. the quantiser (closed form)
        g_res0 = g_cb = None
        if need_h or need_win or need_cb:
            sink = ctx.grad_sink
            out_cb = None
            if need_cb and sink is not None and tuple(sink.view.shape) == tuple(codebooks.shape) and all(
                    p.grad is None and getattr(p, "_rq_sink_epoch", -1) != sink.owner.epoch for p in sink.params):
                out_cb = sink.view
                for p in sink.params:
                    p._rq_sink_epoch = sink.owner.epoch
            g_res0, g_cb = ops.rq_backward(res0, codebooks, ctx.mode, ctx.beta, ids, g_embsum=g_es, g_loss=g_loss,
                                           need_res0=need_h or need_win, need_codebooks=need_cb, out_g_codebooks=out_cb,
                                           cbgrad=ops.cbgrad_default())
            if out_cb is not None and g_cb is not None:
                g_cb = g_cb.view_as(g_cb)
        # 3. encoder side: res0 = h w_in^T, h = relu(...) of the encoder stack's last layer
        g_h = None
        if g_res0 is not None and need_win:
            if jobs:
                pending.append(_lin.WgradJob(w_in, g_res0, h, None, None, claim_grad_sink(w_in)))
            else:
                sink = claim_grad_sink(w_in)
                gw, _, _ = _lin.weight_grad(g_res0, None, h, w_in, out=sink)
                gw_in = gw.view_as(gw) if sink is not None else gw
        for j, gw in zip(pending, _lin.launch_wgrads(pending)):
            gw = gw.view_as(gw) if j.sink is not None else gw
            if j.w is w_out:
                gw_out = gw
            else:
                gw_in = gw
        if g_res0 is not None and need_h:
            cols = None
            if ctx.want_scales:      # the forward's spare half, once; a second backward through a retained graph zeroes its own
                cols, ctx.bwd_cols = ctx.bwd_cols, None
                if cols is None:
                    cols = _lin.zeros_i32(ops.SEAM_H, h.device)
            g_h, sc = _lin.chain_input_grad(g_res0, w_in, out_mask=h, want_rows=ctx.want_scales, col_out=cols)
            _lin.handoff_grad(g_h, sc if ctx.want_scales else _lin.Scales())
        return g_h, gw_in, g_cb, gw_out, None, None, None, None


class GumbelLevelFunction(torch.autograd.Function):
    """One GUMBEL_SOFTMAX level (training): forward(x [B,D], codebook [K,D], U [B,K], T, beta) -> emb, ids, loss."""

    @staticmethod
    def forward(ctx, x: Tensor, codebook: Tensor, U: Tensor, temperature: float, beta: float):
        ids, emb, loss = ops.gumbel_forward(x, codebook, U, temperature, beta)
        ctx.save_for_backward(x, codebook, U)
        ctx.temperature, ctx.beta = temperature, beta
        ctx.mark_non_differentiable(ids)
        return emb, ids, loss

    @staticmethod
    def backward(ctx, g_emb, _g_ids, g_loss):
        x, codebook, U = ctx.saved_tensors
        g_x, g_cb = ops.gumbel_backward(x, codebook, U, ctx.temperature, ctx.beta, g_emb=_dense(g_emb),
                                        g_loss=_dense(g_loss))
        return g_x, g_cb, None, None, None


# The factor the caller will apply to the batch-mean loss before calling backward() (1 / gradient_accumulate_every, or a
# micro-batch's share of a larger batch).  Only a HINT for the speculative reconstruction-loss gradient below: a wrong
# value costs the saved pass, never correctness.
_LOSS_SCALE = 1.0


class loss_scale:
    """`with loss_scale(s): out = model(batch, t)` -- tell the forward that `out.loss * s` is what will be backpropagated."""

    def __init__(self, s: float) -> None:
        self.s, self.prev = float(s), 1.0

    def __enter__(self):
        global _LOSS_SCALE
        self.prev, _LOSS_SCALE = _LOSS_SCALE, self.s
        return self

    def __exit__(self, *exc):
        global _LOSS_SCALE
        _LOSS_SCALE = self.prev
        return False


class ReconLossFunction(torch.autograd.Function):
    """Row-wise squared error (reference modules/loss.py:5-10) as one HIP pass forward and one backward.

    When only x_hat needs a gradient (the training step), the forward pass also writes the gradient it expects to be
    asked for -- 2 (x_hat - x) / B, what `.mean().backward()` of rqvae.py:152-154 sends -- and the backward pass merely
    verifies the upstream rows on the device, redoing the ones that differ: same results, one pass over the [B, 768]
    tensors instead of two."""

    @staticmethod
    def forward(ctx, x_hat: Tensor, x: Tensor):
        B = x.shape[0]
        ctx.spec = B > 0 and ctx.needs_input_grad[0] and not ctx.needs_input_grad[1] and ops.recon_spec_ok(x_hat, x)
        if ctx.spec:
            # fp32 (loss scale) * fp32 (1 / B): what autograd's multiply + mean backward hand to every row on the device
            # (a scalar divisor becomes a multiplication by its fp32 reciprocal there, and in rqhip_loss_means_backward)
            one = torch.tensor(1.0, dtype=torch.float32)
            ctx.row_scale = float(torch.tensor(_LOSS_SCALE, dtype=torch.float32) * (one / B))
            out, g_spec = ops.recon_loss_forward_spec(x_hat, x, ctx.row_scale)
            ctx.save_for_backward(x_hat, x, g_spec)
            return out
        ctx.save_for_backward(x_hat, x)
        return ops.recon_loss_forward(x_hat, x)

    @staticmethod
    def backward(ctx, g_out):
        if ctx.spec and not getattr(ctx, "spec_consumed", False):
            # the speculative buffer is handed to autograd (and fixed up in place) ONCE; a second backward through a
            # retained graph recomputes from x_hat and x below instead of returning the first call's tensor again
            ctx.spec_consumed = True
            x_hat, x, g_spec = ctx.saved_tensors
            return ops.recon_loss_backward_spec(x_hat, x, _dense(g_out), ctx.row_scale, g_spec), None
        x_hat, x = ctx.saved_tensors[:2]
        need_hat, need_x = ctx.needs_input_grad
        if not (need_hat or need_x):
            return None, None
        return ops.recon_loss_backward(x_hat, x, _dense(g_out), need_hat, need_x)


class LossMeansFunction(torch.autograd.Function):
    """(loss, reconstruction_loss, rqvae_loss) of RqVae.forward -- mean(recon + quant), mean(recon), mean(quant) -- as one
    launch.  Backward is what autograd derives for the three means, also one launch: every row of `recon` receives
    (g_loss + g_recon_mean) * (1/B), every row of `quant` (g_loss + g_quant_mean) * (1/B)."""

    @staticmethod
    def forward(ctx, recon: Tensor, quant: Tensor):
        ctx.n = recon.numel()
        ctx.set_materialize_grads(False)   # unused means arrive as None, not as zero tensors to add
        out = ops.loss_means(recon, quant)
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, g_loss, g_rmean, g_qmean):
        need_r = ctx.needs_input_grad[0] and (g_loss is not None or g_rmean is not None)
        need_q = ctx.needs_input_grad[1] and (g_loss is not None or g_qmean is not None)
        if g_rmean is None and g_qmean is None and g_loss is not None and need_r and need_q:
            rows, _ = ops.loss_means_backward(g_loss, None, None, ctx.n, True, False)
            return rows, rows       # the usual case (only `loss` is backpropagated): one vector serves both inputs
        return ops.loss_means_backward(g_loss, g_rmean, g_qmean, ctx.n, need_r, need_q)


class T5AttentionFunction(torch.autograd.Function):
    """One T5 attention call (modules/t5.py:_attend with its head transposes) as one launch forward and one attention
    launch backward (ops.t5_attention_fwd_train / ops.t5_attention_bwd): q [R, Tq, heads * 64], k / v [R, Tk, heads * 64],
    the relative-position bias as a table by j - i.  The weights are recomputed in the backward, the dropout decisions
    (p > 0, `seed`: a one-element int64 device tensor) too; only q, k, v, out and the row log-sum-exp are saved.
    Gradients: q, k, v and the table (whose own graph leads to relative_attention_bias.weight)."""

    @staticmethod
    def forward(ctx, q: Tensor, k: Tensor, v: Tensor, bias_by_delta: Optional[Tensor], n_heads: int, bias_offset: int,
                key_mask: Optional[Tensor], causal: bool, p: float, seed: Optional[Tensor]):
        out, lse = ops.t5_attention_fwd_train(q, k, v, n_heads, bias_by_delta=bias_by_delta, bias_offset=bias_offset,
                                              key_mask=key_mask, causal=causal, p=p, seed=seed)
        ctx.save_for_backward(q, k, v, out, lse, bias_by_delta, key_mask, seed)
        ctx.call = (n_heads, bias_offset, causal, p)
        return out

    @staticmethod
    def backward(ctx, d_out: Tensor):
        q, k, v, out, lse, table, mask, seed = ctx.saved_tensors
        n_heads, bias_offset, causal, p = ctx.call
        dq, dk, dv, dtable = ops.t5_attention_bwd(q, k, v, out, lse, d_out, n_heads, bias_by_delta=table,
                                                  bias_offset=bias_offset, key_mask=mask, causal=causal, p=p, seed=seed)
        return dq, dk, dv, dtable, None, None, None, None, None, None


class T5AttentionPackedFunction(torch.autograd.Function):
    """T5AttentionFunction on packed variable-length rows (ops.t5_attention_packed_fwd_train / _bwd): apply(q, k, v,
    bias_by_delta or None, n_heads, bias_offset, cu_q or None, cu_k or None, max_q, max_k, p, seed).  A side with its
    int32 table is 2-D [rows, heads * 64], a side without the dense [groups, T, heads * 64]; max_q / max_k are the padded
    lengths, whose index laws the bias and the dropout keep.  Saved: q, k, v, out, the row log-sum-exp, the table of the
    bias, the two cumulative tables and the seed.  Gradients: q, k, v and the bias table."""

    @staticmethod
    def forward(ctx, q: Tensor, k: Tensor, v: Tensor, bias_by_delta: Optional[Tensor], n_heads: int, bias_offset: int,
                cu_q: Optional[Tensor], cu_k: Optional[Tensor], max_q: int, max_k: int, p: float,
                seed: Optional[Tensor]):
        out, lse = ops.t5_attention_packed_fwd_train(q, k, v, n_heads, cu_q=cu_q, cu_k=cu_k, max_q=max_q, max_k=max_k,
                                                     bias_by_delta=bias_by_delta, bias_offset=bias_offset, p=p, seed=seed)
        ctx.save_for_backward(q, k, v, out, lse, bias_by_delta, cu_q, cu_k, seed)
        ctx.call = (n_heads, bias_offset, max_q, max_k, p)
        return out

    @staticmethod
    def backward(ctx, d_out: Tensor):
        q, k, v, out, lse, table, cu_q, cu_k, seed = ctx.saved_tensors
        n_heads, bias_offset, max_q, max_k, p = ctx.call
        dq, dk, dv, dtable = ops.t5_attention_packed_bwd(q, k, v, out, lse, d_out, n_heads, cu_q=cu_q, cu_k=cu_k,
                                                         max_q=max_q, max_k=max_k, bias_by_delta=table,
                                                         bias_offset=bias_offset, p=p, seed=seed)
        return (dq, dk, dv, dtable) + (None,) * 8


class RowsPackFunction(torch.autograd.Function):
    """Padded rows [B, T, d] -> packed rows [N, d] (ops.rows_pack): apply(x, cu, N) with cu the int32 [B + 1] device
    table and N the host's row count.  Its backward is ops.rows_unpack of the gradient: zero on the padded tails."""

    @staticmethod
    def forward(ctx, x: Tensor, cu: Tensor, N: int):
        ctx.save_for_backward(cu)
        ctx.shape = (x.shape[0], x.shape[1])
        return ops.rows_pack(x, cu, N)

    @staticmethod
    def backward(ctx, g: Tensor):
        (cu,) = ctx.saved_tensors
        return ops.rows_unpack(_dense(g), cu, *ctx.shape), None, None


class RowsUnpackFunction(torch.autograd.Function):
    """Packed rows [N, d] -> padded rows [B, T, d] with zero tails (ops.rows_unpack): apply(x, cu, B, T).  Its backward
    is ops.rows_pack of the gradient."""

    @staticmethod
    def forward(ctx, x: Tensor, cu: Tensor, B: int, T: int):
        ctx.save_for_backward(cu)
        ctx.n = x.shape[0]
        return ops.rows_unpack(x, cu, B, T)

    @staticmethod
    def backward(ctx, g: Tensor):
        (cu,) = ctx.saved_tensors
        return ops.rows_pack(_dense(g), cu, ctx.n), None, None, None


class T5AttentionLongFunction(torch.autograd.Function):
    """T5AttentionFunction for the lengths beyond its kernel (ops.t5_attention_long_fwd_train / ops.t5_attention_long_bwd,
    up to 2048 tokens): the same arguments and gradients, and a trailing `arith` (ops.T5_ARITHS), the arithmetic of
    forward and backward alike: the (m, l) pair a forward saves is read by the backward of its own arithmetic only.
    Saved: q, k, v, out, the row log-sum-exp, each row's (max, sum) pair, the table, the mask and the seed, all float32
    in both arithmetics; the weights and the dropout decisions are recomputed chunk by chunk."""

    @staticmethod
    def forward(ctx, q: Tensor, k: Tensor, v: Tensor, bias_by_delta: Optional[Tensor], n_heads: int, bias_offset: int,
                key_mask: Optional[Tensor], causal: bool, p: float, seed: Optional[Tensor], arith: str = "fp32"):
        arith_kw = {} if arith == "fp32" else {"arith": arith}      # the keyword only off the ops' default
        out, lse, ml = ops.t5_attention_long_fwd_train(q, k, v, n_heads, bias_by_delta=bias_by_delta,
                                                       bias_offset=bias_offset, key_mask=key_mask, causal=causal, p=p,
                                                       seed=seed, **arith_kw)
        ctx.save_for_backward(q, k, v, out, lse, ml, bias_by_delta, key_mask, seed)
        ctx.call = (n_heads, bias_offset, causal, p, arith_kw)
        return out

    @staticmethod
    def backward(ctx, d_out: Tensor):
        q, k, v, out, lse, ml, table, mask, seed = ctx.saved_tensors
        n_heads, bias_offset, causal, p, arith_kw = ctx.call
        dq, dk, dv, dtable = ops.t5_attention_long_bwd(q, k, v, out, lse, ml, d_out, n_heads, bias_by_delta=table,
                                                       bias_offset=bias_offset, key_mask=mask, causal=causal, p=p,
                                                       seed=seed, **arith_kw)
        return dq, dk, dv, dtable, None, None, None, None, None, None, None


class T5AddNormFunction(torch.autograd.Function):
    """The glue between two T5 sub-layers (modules/t5.py, norm_impl = "hip") as one launch forward and one backward
    (ops.t5_add_norm_fwd / ops.t5_add_norm_bwd): apply(x or None, y, w, eps, p_in, p_out, seed) -> (x_new, n) with
    x_new = x + dropout(y, p_in) and n = dropout(w * rms_norm(x_new), p_out).  Only x_new, the rows' rstd, w and the
    seed are saved; the dropout decisions are recomputed.  Gradients: x, y and w; at p_in = 0 those of x and y are one
    tensor."""

    @staticmethod
    def forward(ctx, x: Optional[Tensor], y: Tensor, w: Tensor, eps: float, p_in: float, p_out: float,
                seed: Optional[Tensor]):
        x_new, n, rstd = ops.t5_add_norm_fwd(x, y, w, eps, p_in, p_out, seed)
        ctx.set_materialize_grads(False)   # an unused output's gradient arrives as None (= NULL at the C ABI)
        ctx.save_for_backward(x_new, rstd, w, seed)
        ctx.call = (p_in, p_out, x is not None)
        return x_new, n

    @staticmethod
    def backward(ctx, d_xnew: Optional[Tensor], d_n: Optional[Tensor]):
        x_new, rstd, w, seed = ctx.saved_tensors
        p_in, p_out, has_x = ctx.call
        if d_xnew is None and d_n is None:
            return None, None, None, None, None, None, None
        d_x, d_y, d_w = ops.t5_add_norm_bwd(x_new, rstd, w, _dense(d_n), _dense(d_xnew), p_in, p_out, seed,
                                            need_x=has_x and ctx.needs_input_grad[0], need_y=ctx.needs_input_grad[1])
        return d_x, d_y, d_w, None, None, None, None


class T5FFNFunction(torch.autograd.Function):
    """The T5 feed-forward body (modules/t5.py, ffn_impl = "hip") as one launch forward and at most two backward
    (ops.t5_ffn_fwd / ops.t5_ffn_bwd): apply(x, wi, wo, p, seed, form=ops.T5_FP32, wi16=None, wo16=None, wi16t=None,
    wo16t=None) -> y = dropout(relu(x @ wi.T), p) @ wo.T, in the arithmetic of `form` (an ops.T5MatmulForm), forward and
    backward alike; every "bf16" form gives the same y and the same gradients, bit for bit.  Gradients: x, wi and wo,
    each only when needed.
    form.images: the forward reads the bf16 weight images wi16 / wo16 (ops.bf16_images) and the backward the transposed
    pair, non-differentiable inputs that must still hold the forward's weights when the backward runs; the gradients go
    to the fp32 weights all the same (the weight-gradient kernel reads no weights).
    Saved: x, the ReLU output h, the two weights and the seed (the dropout decisions are recomputed), with images the
    transposed pair too.  form.saved: instead of x, h and the seed, the blocked bf16 images hd16 of dropout(relu(x @
    wi.T)) and x16 of x -- nothing fp32 of the activations' size; the backward's active set is hd16 > 0."""

    @staticmethod
    def forward(ctx, x: Tensor, wi: Tensor, wo: Tensor, p: float, seed: Optional[Tensor],
                form: ops.T5MatmulForm = ops.T5_FP32, wi16: Optional[Tensor] = None, wo16: Optional[Tensor] = None,
                wi16t: Optional[Tensor] = None, wo16t: Optional[Tensor] = None):
        y, h = ops.t5_ffn_fwd(x, wi, wo, p, seed, **form.keywords((wi16, wo16)))
        kept = (*h, wi, wo) if form.saved else (x, h, wi, wo, seed)
        ctx.save_for_backward(*kept, *((wi16t, wo16t) if form.images else ()))
        ctx.p, ctx.form = p, form
        return y

    @staticmethod
    def backward(ctx, d_y: Tensor):
        need_x, need_wi, need_wo = ctx.needs_input_grad[:3]
        if not (need_x or need_wi or need_wo):
            return (None,) * 10
        form, kept = ctx.form, list(ctx.saved_tensors)
        kw = form.keywords((kept.pop(-2), kept.pop()) if form.images else None)
        if form.saved:
            hd16, x16, wi, wo = kept
            x, h, seed = None, (hd16, x16), None
        else:
            x, h, wi, wo, seed = kept
        d_x, d_wi, d_wo = ops.t5_ffn_bwd(x, wi, wo, h, _dense(d_y), ctx.p, seed, need_x=need_x, need_wi=need_wi,
                                         need_wo=need_wo, **kw)
        return (d_x, d_wi, d_wo) + (None,) * 7


class T5ProjFunction(torch.autograd.Function):
    """A group of bias-free linear maps of the same rows (modules/t5.py, proj_impl = "hip") as one launch forward and at
    most two backward (ops.t5_proj_fwd / ops.t5_proj_bwd): apply(x, form, *tensors) -> (y[0], ..., y[n - 1]), y[j] = x @
    weights[j].T, in the arithmetic of `form` (an ops.T5MatmulForm).  tensors: the n weights; with form.images their n
    bf16 images [d_out, d_in] and their n transposed images [d_in, d_out] follow (non-differentiable inputs; the same
    outputs and gradients, bit for bit; the transposed images must still hold the forward's weights when the backward
    runs).  Saved: x, the weights and the transposed images.  An output nobody used arrives without a gradient and is
    left out of the backward.  Gradients: x and each weight, each only when needed."""

    @staticmethod
    def forward(ctx, x: Tensor, form: ops.T5MatmulForm, *tensors: Tensor):
        n = len(tensors) // 3 if form.images else len(tensors)
        outs = ops.t5_proj_fwd(x, tensors[:n], **form.keywords(tensors[n:2 * n]))
        ctx.set_materialize_grads(False)   # an unused output's gradient arrives as None (= NULL at the C ABI)
        ctx.save_for_backward(x, *tensors[:n], *tensors[2 * n:])
        ctx.form, ctx.n = form, n
        return outs

    @staticmethod
    def backward(ctx, *d_ys: Optional[Tensor]):
        n, need = ctx.n, ctx.needs_input_grad
        x, *rest = ctx.saved_tensors
        if all(g is None for g in d_ys) or not (need[0] or any(need[2:2 + n])):
            return (None,) * len(need)
        d_x, d_w = ops.t5_proj_bwd(x, rest[:n], [_dense(g) for g in d_ys], need_x=need[0], need_w=need[2:2 + n],
                                   **ctx.form.keywords(rest[n:]))
        return (d_x, None, *d_w) + (None,) * (len(need) - 2 - n)      # nothing for the form and the images


class SidHeadLossFunction(torch.autograd.Function):
    """The retrieval model's L semantic-id heads and their cross-entropy losses (modules/model.py, head_impl = "hip") as
    one call forward and one backward (ops.sid_head_loss_fwd / ops.sid_head_loss_bwd): apply(x, target, *weights) ->
    (loss, loss_d) with x the decoder's unsliced [B, T >= L, d] hidden states, target [B, >= L] and L = len(weights)
    separate [K, d] matrices.  loss_d is not differentiable.  Saved: x, target, the weights, the logits z and the rows'
    log-sum-exp.  Gradients: x (dense [B, T, d], zero at the positions no head reads) and each weight that needs one."""

    @staticmethod
    def forward(ctx, x: Tensor, target: Tensor, *weights: Tensor):
        L = len(weights)
        loss, loss_d, z, lse = ops.sid_head_loss_fwd(x, weights, target, L)
        ctx.set_materialize_grads(False)   # without a gradient for `loss` there is nothing to do
        ctx.mark_non_differentiable(loss_d)
        ctx.save_for_backward(x, target, z, lse, *weights)
        return loss, loss_d

    @staticmethod
    def backward(ctx, d_loss: Optional[Tensor], _d_loss_d):
        x, target, z, lse, *weights = ctx.saved_tensors
        L = len(weights)
        if d_loss is None or not any(ctx.needs_input_grad):
            return (None,) * (2 + L)
        d_x, d_w = ops.sid_head_loss_bwd(x, weights, target, z, lse, _dense(d_loss), L,
                                         need_x=ctx.needs_input_grad[0], need_w=ctx.needs_input_grad[2:])
        return (d_x, None, *d_w)


class SidEmbedFunction(torch.autograd.Function):
    """The retrieval model's input embedding (modules/model.py, embed_impl = "hip") as one launch forward and one
    backward (ops.sid_embed_fwd / ops.sid_embed_bwd): apply(ids, mask or None, table, sep or None, prefix_table or None,
    prefix_idx or None, L, ld_item, need_mask) -> (x, mask_out).  mask_out is not differentiable (None without
    need_mask).  Saved: the ids, the mask and the prefix indices, no activation.  Gradients: table, sep (in its own
    shape) and prefix_table, each only when needed."""

    @staticmethod
    def forward(ctx, ids: Tensor, mask: Optional[Tensor], table: Tensor, sep: Optional[Tensor],
                prefix_table: Optional[Tensor], prefix_idx: Optional[Tensor], L: int, ld_item: int, need_mask: bool):
        x, mask_out = ops.sid_embed_fwd(ids, mask, table, L, ld_item, sep, prefix_table, prefix_idx, need_mask=need_mask)
        if prefix_table is None:
            prefix_idx = None
        ctx.set_materialize_grads(False)   # no zero-filled gradient for mask_out; x unused: its gradient arrives as None
        ctx.save_for_backward(ids, mask, prefix_idx)
        ctx.plan = (L, ld_item, table.shape[0] // L, None if sep is None else sep.shape,
                    0 if prefix_table is None else prefix_table.shape[0])
        if mask_out is not None:
            ctx.mark_non_differentiable(mask_out)
        return x, mask_out

    @staticmethod
    def backward(ctx, d_x: Optional[Tensor], _d_mask_out):
        ids, mask, prefix_idx = ctx.saved_tensors
        L, ld_item, K, sep_shape, prefix_rows = ctx.plan
        need_table, need_sep, need_prefix = ctx.needs_input_grad[2:5]
        if d_x is None or not (need_table or need_sep or need_prefix):
            return (None,) * 9
        d_table, d_sep, d_prefix = ops.sid_embed_bwd(_dense(d_x), ids, mask, L, ld_item, K, has_sep=sep_shape is not None,
                                                     prefix_rows=prefix_rows, prefix_idx=prefix_idx,
                                                     need_table=need_table, need_sep=need_sep, need_prefix=need_prefix)
        if d_sep is not None:
            d_sep = d_sep.view(sep_shape)
        return None, None, d_table, d_sep, d_prefix, None, None, None, None
