"""bf16 weight images on the GPU: the image kernel against integer arithmetic on the fp32 bit patterns, the four
image-reading kernels against the "bf16" arithmetic they restate, and `weight_images = "bf16"` on the retrieval model
against `"none"`.

There is no tolerance anywhere in this file.  An image element is the operand the bf16 arm rounds in registers, the
groups, chains and their order are the bf16 arm's, and which lane serves a column does not enter its sum: every output
of the image arm must have the bits of the bf16 arm, which has passed its own error gates (tests/test_gpu_t5_ffn_bf16.py,
tests/test_gpu_t5_proj_bf16.py).  Every comparison is torch.equal on int32 views.

Shapes.  Feed-forward (N, d, F): (1, 32, 32) the smallest; (17, 96, 160) a partial row tile, a partial chunk of F, three
column pairs and so an idle wave; (40, 384, 1024) the model's widths over three row tiles; (33, 512, 64) four column
pairs per wave; (16385, 32, 32) the 32-row tile.  Projections: N = 8193 and 16385 are the first batches of the 32- and
64-row tiles."""
import ctypes as C

import numpy as np
import pytest
import torch

from retrieval_cases import loss_and_grads, same_bits, tiny_model, to_device

pytestmark = pytest.mark.gpu

BF = "bf16"
SENTINEL = 0x5A5A       # a bf16 pattern no test value rounds to: what an image that must not be written holds


# ---- the image kernel

# fp32 patterns whose rounding is a corner: +-0, denormals (the smallest, a halfway value that goes down to zero, one
# that goes up to the even neighbour, the largest negative), exact halfway values that round to even upward (0x3F818000)
# and downward (0x3F808000) and their negatives, just beside halfway, the largest finite values (they round to inf) and
# +-inf
FINITE_CORNERS = (0x00000000, 0x80000000, 0x00000001, 0x00008000, 0x00018000, 0x00008001, 0x807FFFFF, 0x3F818000,
                  0x3F808000, 0xBF818000, 0xBF808000, 0x3F807FFF, 0x3F808001, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000,
                  0x7F7F7FFF, 0x7F800000, 0xFF800000)
NANS = (0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0xFF80FFFF)


def expected_bits(u):
    """bf16 round-to-nearest-even of finite (and infinite) fp32 patterns, in integer arithmetic on the pattern."""
    u = u.astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _matrix(rows, cols, seed, corners=True):
    """A float32 [rows, cols] device matrix of normal draws over many binades, its first elements the corner patterns."""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((rows, cols)) * np.exp2(rng.integers(-20, 20, (rows, cols)))).astype(np.float32)
    u = w.view(np.uint32).reshape(-1)
    if corners:
        pats = FINITE_CORNERS + NANS
        u[:len(pats)] = np.array(pats, dtype=np.uint32)
        u[-1] = 0x3F818000         # the last element of the last tile too
    return torch.from_numpy(u.view(np.float32).reshape(rows, cols).copy()).cuda()


def _u16(img):
    return img.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _check_image(w, img, img_t):
    u = w.cpu().numpy().view(np.uint32)
    got = _u16(img)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    want = expected_bits(u)
    assert got.shape == u.shape
    assert np.array_equal(got[~nan], want[~nan])
    assert bool((((got[nan] & 0x7F80) == 0x7F80) & ((got[nan] & 0x007F) != 0)).all())     # a NaN stays a NaN
    if img_t is not None:
        assert tuple(img_t.shape) == (w.shape[1], w.shape[0])
        assert torch.equal(img_t.view(torch.int16), img.t().contiguous().view(torch.int16))


def _launch(ws, skip_t=()):
    """One launch over `ws` -> (imgs, imgs_t, the transposed views that were NOT handed to the kernel)."""
    from rqhip import ops
    arena, imgs, all_t = ops.bf16_images_alloc(ws)
    arena.view(torch.int16).fill_(SENTINEL)
    imgs_t = [None if j in skip_t else t for j, t in enumerate(all_t)]
    jobs = ops.bf16_images_jobs(ws, imgs, imgs_t)
    assert jobs.n_jobs == len(ws) and jobs.n_tiles == sum(w.numel() // 1024 for w in ws) and jobs.table.is_cuda
    ops.bf16_images(jobs)
    return imgs, imgs_t, [all_t[j] for j in skip_t]


@pytest.mark.parametrize("transposed", [True, False])
@pytest.mark.parametrize("rows,cols", [(32, 32), (96, 64), (384, 1024)])
def test_one_image(rows, cols, transposed):
    w = _matrix(rows, cols, rows + cols)
    keep = w.clone()
    imgs, imgs_t, untouched = _launch([w], skip_t=() if transposed else (0,))
    _check_image(w, imgs[0], imgs_t[0])
    assert (imgs_t[0] is not None) == transposed and torch.equal(w.view(torch.int32), keep.view(torch.int32))
    for t in untouched:
        assert bool((t.view(torch.int16) == SENTINEL).all())


def test_seventy_jobs_of_mixed_shapes_in_one_launch():
    """More jobs than the Amazon model's 64, every third without a transposed image."""
    shapes = [(32, 32), (96, 64), (64, 96), (32, 128), (160, 32)]
    ws = [_matrix(*shapes[j % len(shapes)], seed=100 + j) for j in range(68)]
    ws.insert(5, _matrix(384, 1024, 7))
    ws.insert(40, _matrix(1024, 384, 8))
    assert len(ws) == 70
    skip = tuple(range(1, 70, 3))
    imgs, imgs_t, untouched = _launch(ws, skip_t=skip)
    for w, img, img_t in zip(ws, imgs, imgs_t):
        _check_image(w, img, img_t)
    assert all(bool((t.view(torch.int16) == SENTINEL).all()) for t in untouched)


def test_a_second_launch_follows_the_weights_and_the_alloc_checks_shapes():
    from rqhip import ops
    from rqhip._lib import RqHipError
    w = _matrix(64, 96, 3, corners=False)
    arena, imgs, imgs_t = ops.bf16_images_alloc([w])
    jobs = ops.bf16_images_jobs([w], imgs, imgs_t)
    ops.bf16_images(jobs)
    first = imgs[0].clone()
    w.mul_(3.0)
    ops.bf16_images(jobs)                      # the table holds pointers: the same table, the new values
    _check_image(w, imgs[0], imgs_t[0])
    assert not torch.equal(first.view(torch.int16), imgs[0].view(torch.int16))
    for bad in (torch.zeros(48, 32, device="cuda"), torch.zeros(32, 32, device="cuda", dtype=torch.float64)):
        with pytest.raises(RqHipError, match="multiples of 32"):
            ops.bf16_images_alloc([bad])
    with pytest.raises(RqHipError, match="imgs"):
        ops.bf16_images_jobs([w], [imgs_t[0]], None)          # an image of the transposed shape


# ---- the kernels: the image arm against the bf16 arm


def _halfway(t, index):
    """t with t[index] moved to exact halfway values between two bf16 neighbours (low half 0x8000), both parities."""
    u = t.cpu().numpy().view(np.uint32).copy()
    u[index] = (u[index] & np.uint32(0xFFFF0000)) | np.uint32(0x8000)
    return torch.from_numpy(u.view(np.float32)).cuda()


def _images_of(ws):
    from rqhip import ops
    arena, imgs, imgs_t = ops.bf16_images_alloc(ws)
    ops.bf16_images(ops.bf16_images_jobs(ws, imgs, imgs_t))
    return imgs, imgs_t


def _same(name, got, want):
    assert len(got) == len(want), name
    for k, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None), f"{name} [{k}]"
        if a is not None:
            assert same_bits(a, b), f"{name} [{k}]"


def _ffn_data(N, d, F, seed, halfway=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(N, d, device="cuda", generator=g)
    wi = torch.randn(F, d, device="cuda", generator=g) * d ** -0.5
    wo = torch.randn(d, F, device="cuda", generator=g) * F ** -0.5
    d_y = torch.randn(N, d, device="cuda", generator=g)
    if halfway:       # a column of each weight
        wi, wo = _halfway(wi, (slice(None), 5)), _halfway(wo, (slice(None), F - 3))
    return x, wi, wo, d_y


def _ffn_both(N, d, F, p, halfway=False):
    from rqhip import ops
    x, wi, wo, d_y = _ffn_data(N, d, F, 7 * N + d + F, halfway)
    seed = torch.tensor([1234 + N], dtype=torch.int64, device="cuda") if p else None
    (wi16, wo16), (wi16t, wo16t) = _images_of([wi, wo])
    name = f"ffn N={N} d={d} F={F} p={p}"
    with torch.no_grad():
        y, h = ops.t5_ffn_fwd(x, wi, wo, p, seed, arith=BF)
        y_i, h_i = ops.t5_ffn_fwd(x, wi, wo, p, seed, arith=BF, w_images=(wi16, wo16))
        _same(name + " forward", (y_i, h_i), (y, h))
        y_n, h_n = ops.t5_ffn_fwd(x, wi, wo, p, seed, need_h=False, arith=BF, w_images=(wi16, wo16))
        assert h_n is None and same_bits(y_n, y), name
        want = ops.t5_ffn_bwd(x, wi, wo, h, d_y, p, seed, return_g=True, arith=BF)
        got = ops.t5_ffn_bwd(x, wi, wo, h, d_y, p, seed, return_g=True, arith=BF, w_images=(wi16t, wo16t))
        _same(name + " backward", got, want)
        # d_x alone (no workspace, g is not stored) and the weight gradients alone
        only_x = ops.t5_ffn_bwd(x, wi, wo, h, d_y, p, seed, need_wi=False, need_wo=False, arith=BF,
                                w_images=(wi16t, wo16t))
        assert same_bits(only_x[0], want[0]) and only_x[1] is None and only_x[2] is None, name
        only_w = ops.t5_ffn_bwd(x, wi, wo, h, d_y, p, seed, need_x=False, arith=BF, w_images=(wi16t, wo16t))
        assert only_w[0] is None and same_bits(only_w[1], want[1]) and same_bits(only_w[2], want[2]), name
    assert bool(torch.isfinite(y).all()) and bool(y.any()) and bool(want[0].any()), name
    return y


FFN_SHAPES = [(1, 32, 32), (17, 96, 160), (40, 384, 1024), (33, 512, 64), (16385, 32, 32)]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("N,d,F", FFN_SHAPES)
def test_feed_forward_has_the_bits_of_the_bf16_arm(N, d, F, p):
    _ffn_both(N, d, F, p)


def test_feed_forward_with_halfway_weights():
    """A column of wi and of wo holds exact halfway values: register rounding and image rounding must agree on ties."""
    _ffn_both(40, 96, 160, 0.1, halfway=True)


def test_feed_forward_reads_the_images_and_not_the_weights():
    """Images of OTHER weights give the bf16 arm's result on those weights: the fp32 weights are not read."""
    from rqhip import ops
    x, wi, wo, d_y = _ffn_data(17, 64, 96, 5)
    wi2, wo2 = wi * 1.5, wo * 0.75
    (wi16, wo16), (wi16t, wo16t) = _images_of([wi2, wo2])
    with torch.no_grad():
        y2, h2 = ops.t5_ffn_fwd(x, wi2, wo2, arith=BF)
        y, h = ops.t5_ffn_fwd(x, wi, wo, arith=BF, w_images=(wi16, wo16))
        assert same_bits(y, y2) and same_bits(h, h2)
        assert not same_bits(y, ops.t5_ffn_fwd(x, wi, wo, arith=BF)[0])
        want = ops.t5_ffn_bwd(x, wi2, wo2, h2, d_y, arith=BF)
        _same("other weights", ops.t5_ffn_bwd(x, wi, wo, h2, d_y, arith=BF, w_images=(wi16t, wo16t)), want)


def test_ops_check_the_images():
    from rqhip import ops
    from rqhip._lib import RqHipError
    x, wi, wo, d_y = _ffn_data(4, 32, 64, 1)
    (wi16, wo16), (wi16t, wo16t) = _images_of([wi, wo])
    for images in ((wi16, wo16), (wi16t, wo16t)):
        with pytest.raises(RqHipError, match='arith="bf16"'):
            ops.t5_ffn_fwd(x, wi, wo, w_images=images)
    with pytest.raises(RqHipError, match="bfloat16"):
        ops.t5_ffn_fwd(x, wi, wo, arith=BF, w_images=(wi, wo))                       # the wrong dtype
    with pytest.raises(RqHipError, match="bfloat16"):
        ops.t5_ffn_fwd(x, wi, wo, arith=BF, w_images=(wi16t, wo16t))                 # the backward's: the wrong shape
    with pytest.raises(RqHipError, match="bfloat16"):
        ops.t5_ffn_bwd(x, wi, wo, torch.zeros(4, 64, device="cuda"), d_y, arith=BF, w_images=(wi16, wo16))
    with pytest.raises(RqHipError, match="bfloat16"):
        ops.t5_ffn_fwd(x, wi, wo, arith=BF, w_images=(wi16.cpu(), wo16))             # the wrong device
    with pytest.raises(RqHipError, match="w_images"):
        ops.t5_proj_fwd(x, [wi, wi], arith=BF, w_images=[wi16])                      # one image for two weights
    with pytest.raises(RqHipError, match="bfloat16"):
        ops.t5_proj_fwd(x, [wi], arith=BF, w_images=[wi16t])
    with pytest.raises(RqHipError, match="bfloat16"):
        ops.t5_proj_bwd(x, [wi], [torch.zeros(4, 64, device="cuda")], arith=BF, w_images=[wi16])


def _proj_data(N, d_in, d_out, n, seed, halfway=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(N, d_in, device="cuda", generator=g)
    ws = [torch.randn(d_out, d_in, device="cuda", generator=g) * d_in ** -0.5 for _ in range(n)]
    d_ys = [torch.randn(N, d_out, device="cuda", generator=g) for _ in range(n)]
    if halfway:
        ws = [_halfway(w, (slice(None), 1 + j)) for j, w in enumerate(ws)]
    return x, ws, d_ys


PROJ_SHAPES = [(32, 32), (384, 64), (96, 384)]


@pytest.mark.parametrize("n", [1, 3, 8])
@pytest.mark.parametrize("d_in,d_out", PROJ_SHAPES)
def test_projections_have_the_bits_of_the_bf16_arm(d_in, d_out, n):
    from rqhip import ops
    for N in (1, 17, 8193, 16385):
        name = f"proj N={N} d_in={d_in} d_out={d_out} n={n}"
        x, ws, d_ys = _proj_data(N, d_in, d_out, n, N + d_in + d_out + n, halfway=(N == 17))
        imgs, imgs_t = _images_of(ws)
        with torch.no_grad():
            _same(name + " y", ops.t5_proj_fwd(x, ws, arith=BF, w_images=imgs), ops.t5_proj_fwd(x, ws, arith=BF))
            want_x, want_w = ops.t5_proj_bwd(x, ws, d_ys, arith=BF)
            got_x, got_w = ops.t5_proj_bwd(x, ws, d_ys, arith=BF, w_images=imgs_t)
        assert same_bits(got_x, want_x) and bool(want_x.any()), name
        _same(name + " d_w", got_w, want_w)
        del x, ws, d_ys, imgs, imgs_t, want_x, want_w, got_x, got_w


@pytest.mark.parametrize("N", [17, 8193])
def test_projections_missing_gradients_and_subsets(N):
    """Some d_y[j] None, need_x False, subsets of need_w: the same bits and the same Nones."""
    from rqhip import ops
    d_in, d_out, n = 96, 64, 4
    x, ws, d_ys = _proj_data(N, d_in, d_out, n, 11)
    imgs, imgs_t = _images_of(ws)
    with torch.no_grad():
        for given, need_x, need_w in (([d_ys[0], None, d_ys[2], None], True, None),
                                      ([None, d_ys[1], None, None], True, [True, False, True, True]),
                                      (d_ys, False, [False, True, False, True]),
                                      (d_ys, True, [False] * 4),
                                      ([None] * 4, True, None)):
            want_x, want_w = ops.t5_proj_bwd(x, ws, given, need_x, need_w, arith=BF)
            got_x, got_w = ops.t5_proj_bwd(x, ws, given, need_x, need_w, arith=BF, w_images=imgs_t)
            _same("d_x", [got_x], [want_x])
            _same("d_w", got_w, want_w)


def test_projections_into_a_strided_slab():
    """Outputs written through a row stride larger than d_out, a position of a decode-cache slab among them."""
    from rqhip import ops
    N, d_in, d_out, pad, extra = 33, 64, 96, 8, 3
    x, ws, _ = _proj_data(N, d_in, d_out, 3, 21)
    imgs, _ = _images_of(ws)
    sentinel = -7.25
    with torch.no_grad():
        dense = ops.t5_proj_fwd(x, ws, arith=BF)
        buf = torch.full((N + extra, d_out + pad), sentinel, device="cuda")
        slab = torch.full((4, N + extra, d_out), sentinel, device="cuda")
        outs = ops.t5_proj_fwd(x.view(N, 1, d_in), ws, [None, buf[:N, :d_out], slab[2, :N]], arith=BF, w_images=imgs)
    assert same_bits(outs[0].view(N, d_out), dense[0])
    assert same_bits(buf[:N, :d_out], dense[1]) and same_bits(slab[2, :N], dense[2])
    assert bool((buf[:, d_out:] == sentinel).all()) and bool((buf[N:] == sentinel).all())
    assert bool((slab[2, N:] == sentinel).all()) and bool((slab[[0, 1, 3]] == sentinel).all())


def test_projections_with_a_row_stride_of_x_at_the_c_interface():
    """ld_x > d_in: ops hands the kernels dense rows, so this goes through the C entry points, both arms on one wide x."""
    from rqhip import _lib, ops
    N, d_in, d_out, n, pad = 19, 64, 96, 2, 12
    x, ws, d_ys = _proj_data(N, d_in, d_out, n, 31)
    imgs, imgs_t = _images_of(ws)
    wide = torch.full((N, d_in + pad), 3.5, device="cuda")
    wide[:, :d_in] = x
    l = _lib.lib()
    vp, i64 = C.c_void_p * n, C.c_int64 * n

    def run(suffix, fwd_w, bwd_w):
        ys = [torch.empty(N, d_out, device="cuda") for _ in range(n)]
        d_x = torch.empty(N, d_in, device="cuda")
        d_w = [torch.empty(d_out, d_in, device="cuda") for _ in range(n)]
        rc = getattr(l, "rqhip_t5_proj_fwd" + suffix)(wide.data_ptr(), d_in + pad, vp(*[w.data_ptr() for w in fwd_w]),
                                                      vp(*[y.data_ptr() for y in ys]), i64(*([d_out] * n)), n, N, d_in,
                                                      d_out, ops._stream())
        assert rc == 0, l.rqhip_last_error()
        rc = getattr(l, "rqhip_t5_proj_bwd" + suffix)(wide.data_ptr(), d_in + pad, vp(*[w.data_ptr() for w in bwd_w]),
                                                      vp(*[g.data_ptr() for g in d_ys]), i64(*([d_out] * n)), n, N, d_in,
                                                      d_out, d_x.data_ptr(), vp(*[g.data_ptr() for g in d_w]),
                                                      ops._stream())
        assert rc == 0, l.rqhip_last_error()
        return ys + [d_x] + d_w

    want, got = run("_bf16", ws, ws), run("_bf16w", imgs, imgs_t)
    _same("ld_x", got, want)
    with torch.no_grad():      # and the wide call is the dense call
        _same("dense", want[:n], ops.t5_proj_fwd(x, ws, arith=BF))


def test_functions_match_their_bf16_twins():
    from rqhip import ops
    from rqhip.autograd import T5FFNFunction, T5ProjFunction
    x, wi, wo, d_y = _ffn_data(26, 64, 96, 9)
    (wi16, wo16), (wi16t, wo16t) = _images_of([wi, wo])
    seed = torch.tensor([77], dtype=torch.int64, device="cuda")
    grads = []
    for images in ((), (wi16, wo16, wi16t, wo16t)):
        leaves = [t.clone().requires_grad_() for t in (x.view(2, 13, 64), wi, wo)]
        y = T5FFNFunction.apply(*leaves, 0.1, seed, ops.T5_BF16_IMAGES if images else ops.T5_BF16, *images)
        y.backward(d_y.view(2, 13, 64))
        grads.append([y.detach()] + [t.grad for t in leaves])
    _same("ffn function", grads[1], grads[0])
    x, ws, d_ys = _proj_data(26, 64, 96, 3, 10)
    imgs, imgs_t = _images_of(ws)
    grads = []
    for use in (False, True):
        leaves = [t.clone().requires_grad_() for t in [x] + ws]
        if use:
            outs = T5ProjFunction.apply(leaves[0], ops.T5_BF16_IMAGES, *leaves[1:], *imgs, *imgs_t)
        else:
            outs = T5ProjFunction.apply(leaves[0], ops.T5_BF16, *leaves[1:])
        torch.autograd.backward([outs[0], outs[2]], [d_ys[0], d_ys[2]])       # an output nobody used
        assert leaves[2].grad is None
        grads.append([o.detach() for o in outs] + [leaves[0].grad, leaves[1].grad, leaves[3].grad])
    _same("proj function", grads[1], grads[0])


# ---- the model: weight_images = "bf16" against "none"

IMAGE_OPS = ("t5_ffn_fwd", "t5_ffn_bwd", "t5_proj_fwd", "t5_proj_bwd")


def _model(images, seed=0):
    dev = torch.device("cuda")
    m = tiny_model(32, 32)
    if seed:       # other weights than tiny_model's own
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.02 * torch.randn(p.shape, generator=g))
    m = m.to(dev)
    m.attention_impl, m.norm_impl, m.head_impl = "hip_train", "hip", "hip"
    m.ffn_impl, m.proj_impl, m.matmul_arith = "hip", "hip", "bf16"
    m.weight_images = "bf16" if images else "none"
    return m


def _batch(seed, B=2):
    from data.schemas import TokenizedSeqBatch
    g = torch.Generator().manual_seed(seed)
    return to_device(TokenizedSeqBatch(torch.zeros(B, 1, dtype=torch.long), torch.randint(0, 16, (B, 8), generator=g),
                                       torch.randint(0, 16, (B, 4), generator=g), torch.ones(B, 8, dtype=torch.bool),
                                       None, None), torch.device("cuda"))


def _stacks(m):
    return (m.encoder.encoder, m.t5_decoder)


def _refreshes(m):
    return [s.images.refreshes for s in _stacks(m)]


def _count(monkeypatch):
    """Every call of the four ops: how many read images, how many do not."""
    import modules.t5 as t5
    calls = {name: {"images": 0, "plain": 0} for name in IMAGE_OPS}
    for name in IMAGE_OPS:
        def counted(*a, _name=name, _real=getattr(t5.ops, name), **kw):
            assert kw.get("arith") == "bf16"
            calls[_name]["images" if kw.get("w_images") is not None else "plain"] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(t5.ops, name, counted)
    return calls


def _eval_loss(m, batch):
    with torch.no_grad():
        return m.eval()(batch).loss


def test_train_step_and_generate_keep_their_bits(monkeypatch):
    calls = _count(monkeypatch)
    batch = _batch(1)
    plain, imaged = _model(False).train(), _model(True).train()
    want_loss, want = loss_and_grads(plain, batch, seed=3)
    n_plain = {k: v["plain"] for k, v in calls.items()}
    assert all(v["images"] == 0 for v in calls.values()) and all(n > 0 for n in n_plain.values())
    assert _refreshes(plain) == [0, 0] and plain.encoder.encoder.images.key is None
    for c in calls.values():
        c.update(images=0, plain=0)
    got_loss, got = loss_and_grads(imaged, batch, seed=3)
    # the same calls, every one of them on the images, after one refresh per stack that drew no random numbers: the
    # dropout seeds behind the same torch.manual_seed, and with them every bit below, are those of the other arm
    assert {k: v["images"] for k, v in calls.items()} == n_plain and all(v["plain"] == 0 for v in calls.values())
    assert _refreshes(imaged) == [1, 1] and imaged.t5_decoder.config.dropout_rate > 0
    assert same_bits(got_loss, want_loss) and sorted(got) == sorted(want) and len(got) > 20
    for name in want:
        assert same_bits(got[name], want[name]), name
    # the holder: one arena per stack, nothing in the state dict
    assert sorted(imaged.state_dict()) == sorted(plain.state_dict())
    for stack in _stacks(imaged):
        n = len(stack.image_weights(True, True))
        assert stack.images.arena.dtype == torch.bfloat16 and stack.images.jobs.n_jobs == n and len(stack.images.pairs) == n
        assert stack.images.arena.numel() == 2 * sum(w.numel() for w in stack.image_weights(True, True))
    assert len(imaged.t5_decoder.image_weights(True, True)) == 4 + 4 + 2      # the cross-attention's weights included
    # generate, exact search: ids and scores
    for m in (plain, imaged):
        m.eval()
        m.beam_impl = "exact"
    for c in calls.values():
        c.update(images=0, plain=0)
    a = plain.generate_next_sem_id(batch)
    n_plain = {k: v["plain"] for k, v in calls.items()}
    for c in calls.values():
        c.update(images=0, plain=0)
    b = imaged.generate_next_sem_id(batch)
    assert {k: v["images"] for k, v in calls.items()} == n_plain and all(v["plain"] == 0 for v in calls.values())
    assert n_plain["t5_proj_fwd"] > 0 and n_plain["t5_ffn_fwd"] > 0
    assert torch.equal(a.sem_ids, b.sem_ids) and same_bits(a.log_probas, b.log_probas)
    assert _refreshes(imaged) == [1, 1]          # the same weights: no further launch


def test_two_eval_forwards_refresh_once():
    m, batch = _model(True).eval(), _batch(2)
    assert _refreshes(m) == [0, 0]
    first = _eval_loss(m, batch)
    assert _refreshes(m) == [1, 1]
    again = _eval_loss(m, batch)
    assert _refreshes(m) == [1, 1] and same_bits(first, again)
    assert same_bits(first, _eval_loss(_model(False), batch))
    # the attribute off, or the other arithmetic: the holder is left alone
    m.matmul_arith = "fp32"
    _eval_loss(m, batch)
    m.matmul_arith, m.weight_images = "bf16", "none"
    assert same_bits(_eval_loss(m, batch), first) and _refreshes(m) == [1, 1]


def _step_both(plain, imaged, batch, make_optimizer, seed):
    for m, opt in ((imaged, make_optimizer(imaged)), (plain, make_optimizer(plain))):
        loss_and_grads(m.train(), batch, seed=seed)
        opt.step()
        m.zero_grad(set_to_none=True)


@pytest.mark.parametrize("kind", ["flat_adamw", "torch_adamw", "load_state_dict"])
def test_stale_images_are_never_read(kind):
    """After the weights change, the next forward equals the "none" arm on the same weights -- and not the old loss,
    which an implementation that caches without the key returns."""
    from rqhip.optim import FlatAdamW
    batch = _batch(4)
    plain, imaged = _model(False), _model(True)
    before = _eval_loss(imaged, batch)
    assert same_bits(before, _eval_loss(plain, batch)) and _refreshes(imaged) == [1, 1]
    if kind == "load_state_dict":
        other = {k: v.clone() for k, v in _model(False, seed=5).state_dict().items()}
        for m in (plain, imaged):
            m.load_state_dict(other)
    else:
        make = ((lambda m: FlatAdamW(m.parameters(), lr=0.05)) if kind == "flat_adamw"
                else (lambda m: torch.optim.AdamW(m.parameters(), lr=0.05)))
        _step_both(plain, imaged, batch, make, seed=6)
    assert _refreshes(imaged) == [1, 1]      # (an optimizer arm's training forward saw the weights of the refresh)
    for a, b in zip(plain.parameters(), imaged.parameters()):
        assert same_bits(a, b)
    want, got = _eval_loss(plain, batch), _eval_loss(imaged, batch)
    assert _refreshes(imaged) == [2, 2]
    assert same_bits(got, want) and not same_bits(got, before)


def test_three_training_steps_leave_the_same_parameters():
    from rqhip.optim import FlatAdamW
    plain, imaged = _model(False).train(), _model(True).train()
    for m in (plain, imaged):
        opt = FlatAdamW(m.parameters(), lr=0.01, max_grad_norm=1.0)
        torch.manual_seed(11)
        for it in range(3):
            loss_and_grads(m, _batch(20 + it), seed=None)
            opt.step()
    assert _refreshes(imaged) == [3, 3]
    names = [n for n, _ in plain.named_parameters()]
    for name, a, b in zip(names, plain.parameters(), imaged.parameters()):
        assert same_bits(a, b), name
    moved = [n for n, p in imaged.named_parameters() if p.grad is not None]
    assert len(moved) > 20


def test_moving_the_model_drops_the_images():
    m, batch = _model(True).eval(), _batch(3)
    want = _eval_loss(m, batch)
    m.float()                                    # _apply: the holder forgets
    assert all(s.images.key is None and s.images.arena is None for s in _stacks(m))
    assert same_bits(_eval_loss(m, batch), want) and _refreshes(m) == [2, 2]
    for s in _stacks(m):
        s.images.invalidate()
    assert same_bits(_eval_loss(m, batch), want) and _refreshes(m) == [3, 3]
