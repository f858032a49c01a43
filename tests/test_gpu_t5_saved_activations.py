"""bf16 saved activations of the "bf16" feed-forward on the GPU: the images' contents against integer arithmetic on the
bf16 arm's fp32 tensors, every output against the bf16 arm, the bytes the autograd Function saves, and
`saved_activations = "bf16"` on the retrieval model against `"fp32"`.

There is no tolerance anywhere in this file.  hd16 holds bf16(keep ? h * s : 0), the only form in which the bf16 arm
feeds h to a matrix instruction, and hd16 > 0 is that arm's active set h > 0 and keep wherever h * s does not round to
zero; g, x and d_y enter the weight gradients only rounded.  So every output must have the bits of the bf16 arm, which
has passed its own error gates (tests/test_gpu_t5_ffn_bf16.py).  Every comparison is torch.equal on integer views.

The one documented difference (include/rqhip.h) is an element with h > 0 that is kept and whose h * s rounds to bf16
zero.  Each case asserts that its reference h has no element with 0 < h * s < 2^-126: h is a sum of 32 or more products
of normal draws, so its positive values are far above the denormals.

Shapes (N, d, F): (1, 32, 32) the smallest; (16, 32, 32) half a block with no writer for the other half; (17, 96, 160)
a partial row tile, a partial chunk of F, three column pairs and so an idle wave; (33, 512, 64) four column pairs and a
block boundary; (40, 384, 1024) the model's widths; (16385, 32, 32) the 32-row tile."""
import functools

import numpy as np
import pytest
import torch

from retrieval_cases import loss_and_grads, same_bits, tiny_model, to_device

pytestmark = pytest.mark.gpu

BF = "bf16"
SHAPES = [(1, 32, 32), (16, 32, 32), (17, 96, 160), (33, 512, 64), (40, 384, 1024), (16385, 32, 32)]


def expected_bits(u):
    """bf16 round-to-nearest-even of finite fp32 patterns, in integer arithmetic on the pattern."""
    u = u.astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _u32(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _rows_u16(img, N, C):
    from rqhip import ops
    return ops.t5_act_image_rows(img, N, C).view(torch.int16).cpu().numpy().view(np.uint16)


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


@functools.lru_cache(maxsize=None)
def _case(N, d, F, p, halfway=False):
    """The data of a case and the bf16 arm's results on it, computed once and left unchanged."""
    from rqhip import ops
    g = torch.Generator(device="cuda").manual_seed(7 * N + d + F)
    x = torch.randn(N, d, device="cuda", generator=g)
    wi = torch.randn(F, d, device="cuda", generator=g) * d ** -0.5
    wo = torch.randn(d, F, device="cuda", generator=g) * F ** -0.5
    d_y = torch.randn(N, d, device="cuda", generator=g)
    if halfway:
        x = _halfway(x, (slice(None), 5))
        parity = (_u32(x)[:, 5] >> 16) & 1
        assert parity.min() == 0 and parity.max() == 1            # ties that round down and ties that round up
    seed = torch.tensor([1234 + N], dtype=torch.int64, device="cuda") if p else None
    with torch.no_grad():
        y, h = ops.t5_ffn_fwd(x, wi, wo, p, seed, arith=BF)
        d_x, d_wi, d_wo, g_ref = ops.t5_ffn_bwd(x, wi, wo, h, d_y, p, seed, return_g=True, arith=BF)
    s = torch.tensor(np.float32(1.0 / (1.0 - p)), device="cuda")       # evaluated in double, rounded once
    hs = h * s if p else h
    # the documented difference cannot occur: no positive h * s below the normal numbers (let alone below 2^-134)
    assert not bool(((hs > 0) & (hs < 2.0 ** -126)).any())
    if p:
        keep = ops.t5_attention_dropout_keep(seed, 1, 1, N, F, p)[0, 0]
        hd = torch.where(keep, hs, torch.zeros_like(hs))
    else:
        hd = hs
    assert bool(torch.isfinite(y).all()) and bool(y.any()) and bool(d_x.any()) and bool((hd > 0).any())
    return dict(x=x, wi=wi, wo=wo, d_y=d_y, seed=seed, y=y, h=h, hd=hd, d_x=d_x, d_wi=d_wi, d_wo=d_wo, g=g_ref)


def _run(N, d, F, p, images, halfway=False):
    from rqhip import ops
    c = _case(N, d, F, p, halfway)
    x, wi, wo, d_y, seed = c["x"], c["wi"], c["wo"], c["d_y"], c["seed"]
    name = f"N={N} d={d} F={F} p={p} images={images}"
    fwd_kw, bwd_kw = {}, {}
    if images:
        (wi16, wo16), (wi16t, wo16t) = _images_of([wi, wo])
        fwd_kw, bwd_kw = {"w_images": (wi16, wo16)}, {"w_images": (wi16t, wo16t)}
    with torch.no_grad():
        y, pair = ops.t5_ffn_fwd(x, wi, wo, p, seed, arith=BF, saved=BF, **fwd_kw)
        hd16, x16 = pair
        assert hd16.dtype == torch.bfloat16 and hd16.numel() == 32 * ((N + 31) // 32) * F, name
        assert x16.dtype == torch.bfloat16 and x16.numel() == 32 * ((N + 31) // 32) * d, name
        assert same_bits(y, c["y"]), name
        # the images: the integer rounding of the bf16 arm's fp32 values
        assert np.array_equal(_rows_u16(hd16, N, F), expected_bits(_u32(c["hd"]))), name + " hd16"
        assert np.array_equal(_rows_u16(x16, N, d), expected_bits(_u32(x))), name + " x16"
        y_n, none = ops.t5_ffn_fwd(x, wi, wo, p, seed, need_h=False, arith=BF, saved=BF, **fwd_kw)
        assert none is None and same_bits(y_n, c["y"]), name

        def bwd(**kw):
            return ops.t5_ffn_bwd(None, wi, wo, pair, d_y, p, None, arith=BF, saved=BF, **bwd_kw, **kw)

        d_x, d_wi, d_wo, g16 = bwd(return_g=True)
        assert same_bits(d_x, c["d_x"]), name + " d_x"
        assert same_bits(d_wi, c["d_wi"]), name + " d_wi"
        assert same_bits(d_wo, c["d_wo"]), name + " d_wo"
        assert np.array_equal(g16.view(torch.int16).cpu().numpy().view(np.uint16), expected_bits(_u32(c["g"]))), name + " g16"
        only_x = bwd(need_wi=False, need_wo=False)            # no workspace
        assert same_bits(only_x[0], c["d_x"]) and only_x[1] is None and only_x[2] is None, name
        only_w = bwd(need_x=False)
        assert only_w[0] is None and same_bits(only_w[1], c["d_wi"]) and same_bits(only_w[2], c["d_wo"]), name
        only_wo = bwd(need_x=False, need_wi=False)            # no room for g16 in the workspace; dy16 is still needed
        assert only_wo[0] is None and only_wo[1] is None and same_bits(only_wo[2], c["d_wo"]), name
        only_wi = bwd(need_x=False, need_wo=False)
        assert only_wi[0] is None and same_bits(only_wi[1], c["d_wi"]) and only_wi[2] is None, name


@pytest.mark.parametrize("images", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("N,d,F", SHAPES)
def test_images_and_outputs_have_the_bits_of_the_bf16_arm(N, d, F, p, images):
    _run(N, d, F, p, images)


@pytest.mark.parametrize("images", [False, True])
def test_a_column_of_x_at_exact_halfway_values(images):
    """Ties in x: the image must round them to even as the bf16 arm's register rounding does, up and down."""
    _run(40, 96, 160, 0.1, images, halfway=True)


def test_the_backward_reads_the_images_and_no_seed():
    """The pair of a forward on OTHER rows gives the bf16 arm's gradients on those rows, at p > 0 without any seed."""
    from rqhip import ops
    c = _case(17, 96, 160, 0.1)
    wi, wo, d_y, seed = c["wi"], c["wo"], c["d_y"], c["seed"]
    x2 = c["x"] * 1.5 + 0.25
    with torch.no_grad():
        _, h2 = ops.t5_ffn_fwd(x2, wi, wo, 0.1, seed, arith=BF)
        want = ops.t5_ffn_bwd(x2, wi, wo, h2, d_y, 0.1, seed, arith=BF)
        _, pair2 = ops.t5_ffn_fwd(x2, wi, wo, 0.1, seed, arith=BF, saved=BF)
        got = ops.t5_ffn_bwd(None, wi, wo, pair2, d_y, 0.1, None, arith=BF, saved=BF)
    for a, b in zip(got, want):
        assert same_bits(a, b)
    assert not same_bits(got[0], c["d_x"]) and not same_bits(got[1], c["d_wi"])


def test_forward_and_backward_replay_from_a_captured_graph():
    """No allocation, copy, memset or sync inside the entry points: both calls capture, and the replay has the bits."""
    from rqhip import ops
    c = _case(17, 96, 160, 0.1)

    def step():
        with torch.no_grad():
            y, pair = ops.t5_ffn_fwd(c["x"], c["wi"], c["wo"], 0.1, c["seed"], arith=BF, saved=BF)
            return (y,) + ops.t5_ffn_bwd(None, c["wi"], c["wo"], pair, c["d_y"], 0.1, None, arith=BF, saved=BF)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for got, name in zip(captured, ("y", "d_x", "d_wi", "d_wo")):
        assert same_bits(got, c[name]), name


def test_ops_check_the_pair():
    from rqhip import ops
    from rqhip._lib import RqHipError
    c = _case(17, 96, 160, 0.0)
    with torch.no_grad():
        _, (hd16, x16) = ops.t5_ffn_fwd(c["x"], c["wi"], c["wo"], arith=BF, saved=BF)
        for pair in ((x16, hd16), (hd16.float(), x16), (hd16[:-32], x16)):
            with pytest.raises(RqHipError, match="bfloat16 image"):
                ops.t5_ffn_bwd(None, c["wi"], c["wo"], pair, c["d_y"], arith=BF, saved=BF)


# ---- the autograd Function: what it saves

def _saved_bytes(fn, args, skip):
    """Bytes of the tensors fn.apply(*args) saves for its backward, without those whose storage is in `skip`."""
    skip = {t.data_ptr() for t in skip if t is not None}
    seen = []

    def pack(t):
        if t.data_ptr() not in skip:
            seen.append(t)
        return t

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        y = fn.apply(*args)
    return y, sum(t.numel() * t.element_size() for t in seen), seen


@pytest.mark.parametrize("images", [False, True])
@pytest.mark.parametrize("N,d,F", [(26, 64, 96), (40, 384, 1024)])
def test_the_function_saves_bf16_images_and_matches_its_fp32_saving_twin(N, d, F, images):
    from rqhip import ops
    from rqhip.autograd import T5FFNFunction
    c = _case(N, d, F, 0.1) if (N, d, F) == (40, 384, 1024) else None
    if c is None:
        g = torch.Generator(device="cuda").manual_seed(9)
        x, wi, wo, d_y = (torch.randn(N, d, device="cuda", generator=g), torch.randn(F, d, device="cuda", generator=g) * d ** -0.5,
                          torch.randn(d, F, device="cuda", generator=g) * F ** -0.5, torch.randn(N, d, device="cuda", generator=g))
    else:
        x, wi, wo, d_y = c["x"], c["wi"], c["wo"], c["d_y"]
    seed = torch.tensor([77], dtype=torch.int64, device="cuda")
    extra = ()
    if images:
        (wi16, wo16), (wi16t, wo16t) = _images_of([wi, wo])
        extra = (wi16, wo16, wi16t, wo16t)
    results, totals = [], []
    for form in (ops.T5MatmulForm(BF, images, False), ops.T5MatmulForm(BF, images, True)):
        leaves = [t.clone().requires_grad_() for t in (x.view(2, N // 2, d), wi, wo)]
        y, total, seen = _saved_bytes(T5FFNFunction, (*leaves, 0.1, seed, form, *extra), skip=(*leaves[1:], seed, *extra))
        y.backward(d_y.view(2, N // 2, d))
        results.append([y.detach()] + [t.grad for t in leaves])
        totals.append(total)
        if form.saved:
            assert all(t.dtype == torch.bfloat16 for t in seen) and len(seen) == 2
    for a, b in zip(results[1], results[0]):
        assert same_bits(a, b)
    assert totals[0] == 4 * N * (d + F)
    assert totals[1] <= 2 * 32 * ((N + 31) // 32) * (d + F)


# ---- the model: saved_activations = "bf16" against "fp32"

NEW_ENTRIES = ("rqhip_t5_ffn_fwd_bf16a", "rqhip_t5_ffn_bwd_bf16a", "rqhip_t5_ffn_fwd_bf16wa", "rqhip_t5_ffn_bwd_bf16wa")


def _model(saved, images, arith="bf16"):
    m = tiny_model(32, 32).to(torch.device("cuda"))
    m.attention_impl, m.norm_impl, m.head_impl = "hip_train", "hip", "hip"
    m.ffn_impl, m.proj_impl, m.matmul_arith = "hip", "hip", arith
    m.weight_images = "bf16" if images else "none"
    m.saved_activations = saved
    return m


def _batch(seed, B=2):
    from data.schemas import TokenizedSeqBatch
    g = torch.Generator().manual_seed(seed)
    return to_device(TokenizedSeqBatch(torch.zeros(B, 1, dtype=torch.long), torch.randint(0, 16, (B, 8), generator=g),
                                       torch.randint(0, 16, (B, 4), generator=g), torch.ones(B, 8, dtype=torch.bool),
                                       None, None), torch.device("cuda"))


def _count(monkeypatch):
    """Every call of the four new C entry points, counted at the library handle the ops look them up on."""
    from rqhip import _lib
    handle = _lib.lib()
    calls = dict.fromkeys(NEW_ENTRIES, 0)
    for name in NEW_ENTRIES:
        def counted(*a, _name=name, _real=getattr(handle, name)):
            calls[_name] += 1
            return _real(*a)
        monkeypatch.setattr(handle, name, counted)
    return calls


@pytest.mark.parametrize("images", [False, True])
def test_a_train_step_keeps_its_loss_and_every_gradient(monkeypatch, images):
    calls = _count(monkeypatch)
    batch = _batch(1)
    fp32, bf16 = _model("fp32", images).train(), _model("bf16", images).train()
    assert bf16.t5_decoder.config.dropout_rate > 0
    want_loss, want = loss_and_grads(fp32, batch, seed=3)
    assert not any(calls.values())
    got_loss, got = loss_and_grads(bf16, batch, seed=3)
    # one feed-forward per block of each stack, forward and backward, all on the arm of this weight_images
    sfx = "wa" if images else "a"
    n_blocks = len(bf16.encoder.encoder.block) + len(bf16.t5_decoder.block)
    assert calls == {name: (n_blocks if name.endswith("_bf16" + sfx) else 0) for name in NEW_ENTRIES}
    assert same_bits(got_loss, want_loss) and sorted(got) == sorted(want) and len(got) > 20
    for name in want:
        assert same_bits(got[name], want[name]), name
    # under no_grad the attribute has no effect: nothing is saved there
    for name in calls:
        calls[name] = 0
    with torch.no_grad():
        assert same_bits(bf16.eval()(batch).loss, fp32.eval()(batch).loss)
    assert not any(calls.values())


@pytest.mark.parametrize("images", [False, True])
def test_three_training_steps_leave_the_same_parameters(images):
    from rqhip.optim import FlatAdamW
    fp32, bf16 = _model("fp32", images).train(), _model("bf16", images).train()
    for m in (fp32, bf16):
        opt = FlatAdamW(m.parameters(), lr=0.01, max_grad_norm=1.0)
        torch.manual_seed(11)
        for it in range(3):
            loss_and_grads(m, _batch(20 + it), seed=None)
            opt.step()
    for (name, a), b in zip(fp32.named_parameters(), bf16.parameters()):
        assert same_bits(a, b), name
    assert len([n for n, p in bf16.named_parameters() if p.grad is not None]) > 20


def test_with_the_fp32_arithmetic_the_attribute_changes_nothing(monkeypatch):
    calls = _count(monkeypatch)
    batch = _batch(2)
    want_loss, want = loss_and_grads(_model("fp32", False, arith="fp32").train(), batch, seed=5)
    got_loss, got = loss_and_grads(_model("bf16", False, arith="fp32").train(), batch, seed=5)
    assert not any(calls.values())
    assert same_bits(got_loss, want_loss) and sorted(got) == sorted(want)
    for name in want:
        assert same_bits(got[name], want[name]), name
