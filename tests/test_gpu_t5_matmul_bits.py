"""The bits of the T5 feed-forward and projection kernels, pinned against a recording (tests/golden/t5_matmul_bits.json).

The other tests of these kernels gate one arm against another with torch.equal, so a change that moves every arm alike
(the group order, the chain rule, a wave's range of blocks, the order of the four waves' sums: csrc/t5_matmul.h) would
pass them all.  Here every output of direct `ops` calls is digested (SHA-256 of the tensor's contiguous CPU bytes) and
compared with the digest the library gave when the fixture was recorded.  The fixture was recorded once, from a library
built at the commit before the matrix code moved into csrc/t5_matmul.h; a digest that differs is a finding about the
kernels, not a reason to record again.  There is no tolerance in this file.

Inputs come from integer arithmetic alone: a multiplicative hash of the element index gives 23 bits k, and the value is
(2 k + 1 - 2^23) / 2^24 * scale, an odd multiple of 2^-24 in (-0.5, 0.5) times a power of two: exact in fp32, never
zero, and independent of any random-number library.

Shapes: the smallest at which each shared piece can go wrong.
  feed-forward (N, d, F, p)
    (17, 32, 32, 0)        one group, a partial row tile
    (33, 160, 160, 0.1)    five groups: a chain of four plus one and an odd round count; two column pairs; a partial
                           second chunk with idle waves; dropout
    (17, 512, 32, 0)       four column pairs
    (1300, 64, 64, 0.1)    waves with more than 8 blocks: several chains per wave and a ragged last block
    (16401, 32, 32, 0)     the 32-row tile
    (16401, 512, 32, 0)    bf16 forms only: the backward that stays on 16-row tiles
  projections (N, d_in, d_out, n)
    (17, 32, 32, 1)        one group, a partial row tile
    (33, 64, 96, 3)        the middle d_y missing and one d_w unwanted; a chain that crosses a segment of d_x's
                           concatenation
    (17, 512, 64, 8)       the largest group count
    (1300, 64, 64, 2)      several chains per wave
    (8209, 32, 32, 1)      the 32-row tile
    (16401, 32, 32, 1)     the 64-row tile
A blocked activation image is digested through ops.t5_act_image_rows, its N specified rows: the rows that pad the last
block are unspecified (include/rqhip.h)."""
import functools
import hashlib
import json
import os

import pytest
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "t5_matmul_bits.json")
SEED = 0x5DEECE66D1CE4E5      # of the inputs and of the dropout decisions

FFN_FORMS = ("T5_FP32", "T5_BF16", "T5_BF16_IMAGES", "T5_BF16_SAVED", "T5_BF16_IMAGES_SAVED")
FFN_SHAPES = ((17, 32, 32, 0.0), (33, 160, 160, 0.1), (17, 512, 32, 0.0), (1300, 64, 64, 0.1), (16401, 32, 32, 0.0),
              (16401, 512, 32, 0.0))
FFN_CASES = [(f, s) for s in FFN_SHAPES for f in FFN_FORMS if not (s == (16401, 512, 32, 0.0) and f == "T5_FP32")]
PROJ_FORMS = ("T5_FP32", "T5_BF16", "T5_BF16_IMAGES")
PROJ_SHAPES = ((17, 32, 32, 1), (33, 64, 96, 3), (17, 512, 64, 8), (1300, 64, 64, 2), (8209, 32, 32, 1),
               (16401, 32, 32, 1))
PROJ_CASES = [(f, s) for s in PROJ_SHAPES for f in PROJ_FORMS]

_M1, _M2 = -7046029254386353131, -4658895280553007687      # 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9 as int64


def values(shape, salt, scale):
    """A float32 device tensor of `shape`: element e is (2 k + 1 - 2^23) / 2^24 * scale, k the top 23 bits of a
    multiplicative hash of e, the salt and SEED (int64 arithmetic, which wraps).  `scale` is a power of two."""
    n = 1
    for s in shape:
        n *= s
    h = (torch.arange(n, dtype=torch.int64) + (SEED + 1000003 * salt)) * _M1
    h = (h ^ ((h >> 29) & ((1 << 35) - 1))) * _M2
    k = (h >> 41) & ((1 << 23) - 1)
    v = (2 * k + 1 - (1 << 23)).to(torch.float32) * (scale / (1 << 24))
    return v.reshape(shape).cuda()


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def _images(weights):
    """The bf16 images of `weights` -> (images, transposed images)."""
    from rqhip import ops
    _arena, imgs, imgs_t = ops.bf16_images_alloc(weights)
    ops.bf16_images(ops.bf16_images_jobs(weights, imgs, imgs_t))
    return imgs, imgs_t


@functools.lru_cache(maxsize=2)
def _ffn_inputs(N, d, F):
    """x, wi, wo, d_y and the images of the weights: computed once per shape and left unchanged."""
    x, wi, wo, d_y = values((N, d), 1, 2.0), values((F, d), 2, 0.5), values((d, F), 3, 0.5), values((N, d), 4, 1.0)
    (wi16, wo16), (wi16t, wo16t) = _images([wi, wo])
    return x, wi, wo, d_y, (wi16, wo16), (wi16t, wo16t)


def ffn_digests(form, shape):
    """Forward and backward of the feed-forward in `form` (a name of FFN_FORMS) -> {output: digest}."""
    from rqhip import ops
    N, d, F, p = shape
    f = getattr(ops, form)
    x, wi, wo, d_y, fwd_images, bwd_images = _ffn_inputs(N, d, F)
    seed = torch.tensor([SEED], dtype=torch.int64, device=x.device) if p else None
    y, h = ops.t5_ffn_fwd(x, wi, wo, p, seed, **f.keywords(fwd_images))
    d_x, d_wi, d_wo, g = ops.t5_ffn_bwd(None if f.saved else x, wi, wo, h, d_y, p, None if f.saved else seed,
                                        return_g=True, **f.keywords(bwd_images))
    out = {"y": y, "d_x": d_x, "d_wi": d_wi, "d_wo": d_wo, "g": g}
    if f.saved:
        out["hd16"], out["x16"] = ops.t5_act_image_rows(h[0], N, F), ops.t5_act_image_rows(h[1], N, d)
    else:
        out["h"] = h
    return {k: digest(v) for k, v in out.items()}


@functools.lru_cache(maxsize=2)
def _proj_inputs(N, d_in, d_out, n):
    x = values((N, d_in), 5, 2.0)
    ws = [values((d_out, d_in), 10 + j, 0.5) for j in range(n)]
    d_ys = [values((N, d_out), 30 + j, 1.0) for j in range(n)]
    imgs, imgs_t = _images(ws)
    return x, ws, d_ys, imgs, imgs_t


def proj_digests(form, shape):
    """Forward and backward of a projection group in `form` (a name of PROJ_FORMS) -> {output: digest}."""
    from rqhip import ops
    N, d_in, d_out, n = shape
    f = getattr(ops, form)
    x, ws, d_ys, imgs, imgs_t = _proj_inputs(N, d_in, d_out, n)
    need_w = [True] * n
    if n == 3:      # the middle d_y missing and the first d_w unwanted: one weight-gradient job, of the last weight
        d_ys, need_w = [d_ys[0], None, d_ys[2]], [False, True, True]
    ys = ops.t5_proj_fwd(x, ws, **f.keywords(imgs))
    d_x, d_w = ops.t5_proj_bwd(x, ws, d_ys, True, need_w, **f.keywords(imgs_t))
    assert [g is not None for g in d_w] == ([False, False, True] if n == 3 else [True] * n)
    out = {f"y{j}": y for j, y in enumerate(ys)}
    out["d_x"] = d_x
    out.update({f"d_w{j}": g for j, g in enumerate(d_w) if g is not None})
    return {k: digest(v) for k, v in out.items()}


def case_id(kind, form, shape):
    return f"{kind}-{form}-" + "x".join(str(s) for s in shape)


def all_digests():
    """Every case -> {case id: {output: digest}}: what the fixture holds."""
    got = {case_id("ffn", f, s): ffn_digests(f, s) for f, s in FFN_CASES}
    got.update({case_id("proj", f, s): proj_digests(f, s) for f, s in PROJ_CASES})
    return got


@functools.lru_cache(maxsize=None)
def _recorded():
    with open(FIXTURE) as fh:
        doc = json.load(fh)
    assert doc["seed"] == SEED
    return doc["digests"]


def test_the_fixture_holds_every_case_and_nothing_else():      # needs no GPU
    want = [case_id("ffn", f, s) for f, s in FFN_CASES] + [case_id("proj", f, s) for f, s in PROJ_CASES]
    assert len(want) == 5 * 5 + 4 + 3 * 6 and sorted(_recorded()) == sorted(want)


@pytest.mark.gpu
@pytest.mark.parametrize("form,shape", FFN_CASES, ids=[case_id("ffn", f, s) for f, s in FFN_CASES])
def test_feed_forward_bits(form, shape):
    got = ffn_digests(form, shape)
    assert len(got) == (7 if "SAVED" in form else 6)
    assert got == _recorded()[case_id("ffn", form, shape)]


@pytest.mark.gpu
@pytest.mark.parametrize("form,shape", PROJ_CASES, ids=[case_id("proj", f, s) for f, s in PROJ_CASES])
def test_projection_bits(form, shape):
    got = proj_digests(form, shape)
    assert len(got) == (3 + 1 + 1 if shape[3] == 3 else 2 * shape[3] + 1)
    assert got == _recorded()[case_id("proj", form, shape)]
