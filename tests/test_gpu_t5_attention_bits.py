"""The bits of the fused T5 attention calls, pinned against a recording (tests/golden/t5_attention_bits.json).

The other attention tests compare one arm with another (packed against padded, fused against the operators within a
tolerance), so a change above the kernels that moves every arm alike -- an argument that reaches the C call copied or with
another stride, another kernel instantiation, launch shape or LDS size, another struct field -- could pass them all.  Here
every output of direct `ops` calls is digested (SHA-256, test_gpu_t5_matmul_bits.digest) and compared with the digest the
library gave when the fixture was recorded: once, from a library and an rqhip/ops.py at the commit before the short
kernels' host calls (csrc/t5_attention.hip) and the nine Python wrappers were given shared bodies.  A digest that differs
is a finding, not a reason to record again.  There is no tolerance in this file.

Inputs are test_gpu_t5_matmul_bits.values: integer arithmetic alone.  The dropout seed has bits above the low 32.
Cases: the smallest that reach each host-side choice.
  padded, R = 3, H = 2 (Tq, Tk):
    (16, 16) causal, bias table, p = 0       MT = 1 and the one-wave arm of forward and backward
    (17, 17) bias table, key mask with one fully masked row, p = 0.1       MT = 6
    (5, 97) key mask, p = 0                  MT = 16, below the 64 KiB LDS grant
    (256, 256) causal, bias table, p = 0.1   the LDS grant
    the (17, 17) case with q, k, v as views of one [R, T, 3 * inner] tensor: the row strides reach the C call uncopied
    inference only: R = 6 over Rk = 2 at (1, 81) (beams); the cached decode step through `anc` at past = 3 on slabs of
    5 positions x 8 rows
  packed, 4 groups of lengths [T, 1, 17, 16], H = 2: the encoder form (both tables, bias table) at T = 17 and 256, p = 0
    and 0.1; the cross form (dense q of 4 tokens, packed K/V, no bias) at T = 81, p = 0.1
  long, R = 2, H = 2, arith "fp32" and "bf16": (7, 300) with a key mask, p = 0; (300, 300) causal with a bias table,
    p = 0.1 (these pin the Python wrappers)
Outputs of a case: the inference call's `out`; the training forward's `out` and `lse` (and `ml`, long); the backward's dq,
dk, dv and, with a bias table, dtable."""
import functools
import json
import os

import pytest
import torch

from test_gpu_t5_matmul_bits import SEED, digest, values

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "t5_attention_bits.json")
H, INNER = 2, 128

#                name: (Tq, Tk, causal, bias, mask, p, views); mask: None, or the row that is wholly masked (-1: none)
PADDED = {"padded-16x16-causal-bias-p0": (16, 16, True, True, None, 0.0, False),
          "padded-17x17-bias-mask-p0.1": (17, 17, False, True, 1, 0.1, False),
          "padded-5x97-mask-p0": (5, 97, False, False, -1, 0.0, False),
          "padded-256x256-causal-bias-p0.1": (256, 256, True, True, None, 0.1, False),
          "padded-17x17-bias-mask-p0.1-views": (17, 17, False, True, 1, 0.1, True)}
INFERENCE = ("beams-6over2-1x81", "decode-past3")
PACKED = {f"packed-encoder-T{T}-p{p}": (T, p) for T in (17, 256) for p in (0.0, 0.1)}
PACKED_CROSS = "packed-cross-T81-p0.1"
#              name: (Tq, Tk, causal, bias, mask, p, arith)
LONG = {f"long-{arith}-{Tq}x{Tk}": (Tq, Tk, causal, bias, mask, p, arith)
        for arith in ("fp32", "bf16")
        for Tq, Tk, causal, bias, mask, p in ((7, 300, False, False, -1, 0.0), (300, 300, True, True, None, 0.1))}
CASES = list(PADDED) + list(INFERENCE) + list(PACKED) + [PACKED_CROSS] + list(LONG)


def _seed(p):
    return torch.tensor([SEED], dtype=torch.int64, device="cuda") if p else None


def _options(Rk, Tq, Tk, causal, bias, mask):
    """The keywords of a dense call.  mask: None, or the row of the bool [Rk, Tk] key mask (integer arithmetic, about a
    fifth masked) that is wholly masked, -1 for none."""
    kw = {"causal": causal}
    if bias:        # one table row per delta j - i of the call
        kw.update(bias_by_delta=values((Tq + Tk - 1, H), 7, 2.0), bias_offset=Tq - 1)
    if mask is not None:
        m = ((torch.arange(Rk * Tk) * 7 + 3) % 5 != 0).view(Rk, Tk)
        if mask >= 0:
            m[mask] = False
        kw["key_mask"] = m.cuda()
    return kw


def _named(names, tensors):
    return {n: digest(t) for n, t in zip(names, tensors) if t is not None}


def _dense(fns, q, k, v, d_out, kw, p, train_kw=None):
    """The three calls of one dense form (fns: inference, fwd_train, bwd) on the same operands -> {output: digest}."""
    inference, fwd_train, bwd = fns
    tkw = dict(kw, p=p, seed=_seed(p), **(train_kw or {}))
    saved = fwd_train(q, k, v, H, **tkw)           # (out, lse) or (out, lse, ml)
    grads = bwd(q, k, v, *saved, d_out, H, **tkw)
    got = {"out": digest(inference(q, k, v, H, **kw, **(train_kw or {})))}
    got.update(_named(("train_out", "lse", "ml"), saved))
    got.update(_named(("dq", "dk", "dv", "dtable"), grads))
    return got


def padded_digests(name):
    from rqhip import ops
    Tq, Tk, causal, bias, mask, p, views = PADDED[name]
    R = 3
    if views:       # q, k, v side by side in one tensor (Tq = Tk): row stride 3 * inner, nothing contiguous
        qkv = values((R, Tq, 3 * INNER), 1, 4.0)
        q, k, v = qkv[..., :INNER], qkv[..., INNER:2 * INNER], qkv[..., 2 * INNER:]
        assert not q.is_contiguous()
    else:
        q, k, v = values((R, Tq, INNER), 1, 4.0), values((R, Tk, INNER), 2, 2.0), values((R, Tk, INNER), 3, 2.0)
    kw = _options(R, Tq, Tk, causal, bias, mask)
    return _dense((ops.t5_attention, ops.t5_attention_fwd_train, ops.t5_attention_bwd), q, k, v,
                  values((R, Tq, INNER), 4, 1.0), kw, p)


def inference_digests(name):
    from rqhip import ops
    if name == "beams-6over2-1x81":
        q, k, v = values((6, 1, INNER), 1, 4.0), values((2, 81, INNER), 2, 2.0), values((2, 81, INNER), 3, 2.0)
        return {"out": digest(ops.t5_attention(q, k, v, H, **_options(2, 1, 81, False, True, -1)))}
    past, positions, slab_rows, R = 3, 5, 8, 6
    ks, vs = values((positions, slab_rows, INNER), 2, 2.0), values((positions, slab_rows, INNER), 3, 2.0)
    anc = ((torch.arange(R * past, dtype=torch.int32) * 5 + 2) % slab_rows).view(R, past).cuda()
    out = ops.t5_attention(values((R, 1, INNER), 1, 4.0), ks, vs, H, bias_by_delta=values((past + 1, H), 7, 2.0),
                           bias_offset=past, past=past, anc=anc)
    return {"out": digest(out)}


def _cu(lengths):
    cu = torch.zeros(len(lengths) + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(torch.tensor(lengths), 0)
    return cu.cuda()


def packed_digests(name):
    from rqhip import ops
    cross = name == PACKED_CROSS
    T, p = (81, 0.1) if cross else PACKED[name]
    lengths = [T, 1, 17, 16]                        # the "mix" of test_gpu_t5_attention_packed.py
    N, cu = sum(lengths), _cu(lengths)
    k, v = values((N, INNER), 2, 2.0), values((N, INNER), 3, 2.0)
    if cross:
        q, d_out = values((4, 4, INNER), 1, 4.0), values((4, 4, INNER), 4, 1.0)
        kw = dict(cu_k=cu, max_k=T)
    else:
        q, d_out = values((N, INNER), 1, 4.0), values((N, INNER), 4, 1.0)
        kw = dict(cu_q=cu, cu_k=cu, max_q=T, max_k=T, bias_by_delta=values((2 * T - 1, H), 7, 2.0), bias_offset=T - 1)
    return _dense((ops.t5_attention_packed, ops.t5_attention_packed_fwd_train, ops.t5_attention_packed_bwd), q, k, v,
                  d_out, kw, p)


def long_digests(name):
    from rqhip import ops
    Tq, Tk, causal, bias, mask, p, arith = LONG[name]
    R = 2
    q, k, v = values((R, Tq, INNER), 1, 4.0), values((R, Tk, INNER), 2, 2.0), values((R, Tk, INNER), 3, 2.0)
    return _dense((ops.t5_attention_long, ops.t5_attention_long_fwd_train, ops.t5_attention_long_bwd), q, k, v,
                  values((R, Tq, INNER), 4, 1.0), _options(R, Tq, Tk, causal, bias, mask), p, {"arith": arith})


def case_digests(name):
    fn = (padded_digests if name in PADDED else inference_digests if name in INFERENCE
          else long_digests if name in LONG else packed_digests)
    return fn(name)


def all_digests():
    """Every case -> {case id: {output: digest}}: what the fixture holds."""
    return {name: case_digests(name) for name in CASES}


@functools.lru_cache(maxsize=None)
def _recorded():
    with open(FIXTURE) as fh:
        doc = json.load(fh)
    assert doc["seed"] == SEED and SEED >> 32
    return doc["digests"]


def test_the_fixture_holds_every_case_and_nothing_else():      # needs no GPU
    assert len(CASES) == 5 + 2 + 4 + 1 + 4 and sorted(_recorded()) == sorted(CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_attention_bits(name):
    got = case_digests(name)
    bias = name in PACKED or "bias" in name or name.endswith("300x300")
    assert len(got) == (1 if name in INFERENCE else 6 + bias + (name in LONG))
    assert got == _recorded()[name]
