"""The retrieval loop's optimizer tail on the device (reference train_decoder.py:147-151, 202-205): rqhip.optim.FlatAdamW with
`max_grad_norm` and modules.scheduler.InverseSquareRootScheduler attached -> csrc/adamw.hip:rqhip_adamw_tail_step (sum of squares,
one scalar kernel, update).  The reference throughout is the whole tail restated below in fp64 on the CPU (`_ref_tail`): clip_grad_norm_'s
coefficient, the inverse-square-root schedule and AdamW.

Tolerances.  Parameters: |ours - fp64| <= 1e-6 max(1, |p|max), the rule of tests/test_gpu_optim.py (torch's own fp32 tail is 2.4e-7 ..
2.7e-7 off the fp64 one on these inputs).  Norm: derived from the shipped reduction, see NORM_ROUNDINGS.  Learning rate: one fp32 ulp."""
import copy
import functools
import math

import pytest
import torch

from retrieval_cases import synthetic_batch, to_device

pytestmark = pytest.mark.gpu

LR, WD, B1, B2, EPS = 1e-2, 1e-2, 0.9, 0.999, 1e-8
SHAPES = [(512, 768), (256, 512), (128, 256), (32, 128), (256, 32), (3,), (1, 1), (1025,)]      # tests/test_gpu_optim.py:_params

# The longest chain of fp32 roundings between one g^2 and the total (csrc/adamw.hip:adamw_sumsq_kernel, adamw_tail_scalars_kernel):
#   1  the square
#   3  the thread's adds of its four squares (vector path; the scalar tail path has at most 3 as well)
#   6  the wave's xor-shuffle tree (64 lanes)
#   2  the workgroup's four wave sums, (w0 + w1) + (w2 + w3)
#   0  the ordered sum of the partials: accumulated in double (its roundings are 2^-53 each), as is the root, which is rounded to
#      fp32 once -- covered by the "one ulp on the root" below
# All terms are non-negative, so the sum is within NORM_ROUNDINGS * 2^-24 (relative) of the exact one, and the root within half of
# that plus one fp32 ulp (2^-23).
NORM_ROUNDINGS = 1 + 3 + 6 + 2
NORM_RTOL = 0.5 * NORM_ROUNDINGS * 2.0 ** -24 + 2.0 ** -23
ULP = 2.0 ** -23


def _family(shapes, steps, seed, none_at=()):
    """(initial parameters, gradients[step][i]) on the CPU: the gradient family of tests/test_gpu_optim.py:_run -- a normal tensor times
    10^k, k uniform in -6 .. 1, drawn per tensor and step."""
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(s, generator=g) for s in shapes]
    g = torch.Generator().manual_seed(seed + 1)
    grads = []
    for _ in range(steps):
        grads.append([None if i in none_at else
                      torch.randn(s, generator=g) * torch.pow(10.0, torch.randint(-6, 2, (1,), generator=g).float())
                      for i, s in enumerate(shapes)])
    return ps, grads


def _ref_tail(ps, grads, max_norm, warmup, lr=LR, wd=WD, m=None, v=None, t0=0):
    """The whole tail in fp64: -> (parameters, norms, lrs, coefs, exp_avg, exp_avg_sq).  `warmup` None: constant lr."""
    ps = [p.double().clone() for p in ps]
    m = [torch.zeros_like(p) for p in ps] if m is None else [x.double().clone() for x in m]
    v = [torch.zeros_like(p) for p in ps] if v is None else [x.double().clone() for x in v]
    norms, lrs, coefs = [], [], []
    for t, gs in enumerate(grads, start=t0 + 1):
        norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in gs if g is not None))
        coef = 1.0 if max_norm is None else min(1.0, max_norm / (norm + 1e-6))
        lr_t = lr if warmup is None or t <= warmup else lr * math.sqrt(warmup) / math.sqrt(t)
        for i, g in enumerate(gs):
            if g is None:
                continue
            g = g.double() * coef
            ps[i] *= 1.0 - lr_t * wd
            m[i] = B1 * m[i] + (1.0 - B1) * g
            v[i] = B2 * v[i] + (1.0 - B2) * g * g
            ps[i] -= (lr_t / (1.0 - B1 ** t)) * m[i] / (v[i].sqrt() / math.sqrt(1.0 - B2 ** t) + EPS)
        norms.append(norm)
        lrs.append(lr_t)
        coefs.append(coef)
    return ps, norms, lrs, coefs, m, v


@functools.lru_cache(maxsize=None)
def _main_case():
    return _family(SHAPES, 7, 0)


@functools.lru_cache(maxsize=None)
def _main_ref(max_norm):
    ps, grads = _main_case()
    return _ref_tail(ps, grads, max_norm, 3)


ODD_NUMELS = [1, 3, 1023, 1024, 1025, 4097] + [5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25, 27, 29, 31, 33, 35, 37, 39, 41, 43, 45, 47, 49, 51]
ODD_NONE, ODD_MISALIGNED = 9, 4          # one tensor without a gradient, one gradient 4 bytes off a 16-byte boundary


@functools.lru_cache(maxsize=None)
def _odd_case():
    assert len(ODD_NUMELS) == 30
    ps, grads = _family([(n,) for n in ODD_NUMELS], 4, 20, none_at=(ODD_NONE,))
    return ps, grads, _ref_tail(ps, grads, 1.0, 2)


def _set_grads(dev_ps, gs, misaligned=()):
    for i, (p, g) in enumerate(zip(dev_ps, gs)):
        if g is None:
            p.grad = None
        elif i in misaligned:
            buf = torch.empty(g.numel() + 1, device="cuda")
            buf[1:].copy_(g.reshape(-1))
            p.grad = buf[1:].view(g.shape)
            assert p.grad.data_ptr() % 16 == 4
        else:
            p.grad = g.cuda()


def _build(ps, max_norm, warmup, lr=LR, wd=WD):
    from modules.scheduler.inv_sqrt import InverseSquareRootScheduler
    from rqhip.optim import FlatAdamW
    dev_ps = [p.cuda().requires_grad_(True) for p in ps]
    opt = FlatAdamW(dev_ps, lr=lr, weight_decay=wd, max_grad_norm=max_norm)
    sched = None if warmup is None else InverseSquareRootScheduler(optimizer=opt, warmup_steps=warmup)
    return dev_ps, opt, sched


def _steps(dev_ps, opt, sched, grads, misaligned=()):
    """optimizer.step() then scheduler.step() per gradient set -> (norms, device lrs, host lrs at step() time), counters checked."""
    norms, dlrs, hlrs = [], [], []
    for gs in grads:
        _set_grads(dev_ps, gs, misaligned)
        hlrs.append(opt.param_groups[0]["lr"])
        if sched is not None:
            assert int(opt.device_lr_step(0)) == sched.last_epoch + 1
        opt.step()
        norms.append(float(opt.grad_norm))
        dlrs.append(float(opt.device_lr(0)))
        if sched is not None:
            sched.step()
    if sched is not None:
        assert int(opt.device_lr_step(0)) == sched.last_epoch + 1
    return norms, dlrs, hlrs


def _close(ours, ref):
    for i, (a, b) in enumerate(zip(ours, ref)):
        err, bound = (a.detach().double().cpu() - b).abs().max().item(), 1e-6 * max(1.0, b.abs().max().item())
        assert err <= bound, (i, err, bound)


def _check_norms_and_lrs(norms, dlrs, hlrs, ref_norms, clip):
    import numpy as np
    for t, (n, rn) in enumerate(zip(norms, ref_norms)):
        print(f"step {t + 1}: norm {n!r} fp64 {rn!r} rel {abs(n - rn) / rn:.3e} (bound {NORM_RTOL:.3e}); lr {dlrs[t]!r} host {hlrs[t]!r}")
        if clip:
            assert abs(n - rn) <= NORM_RTOL * rn, (t, n, rn)
        else:
            assert math.isnan(n)                      # not computed without clipping
        assert abs(dlrs[t] - float(np.float32(hlrs[t]))) <= ULP * hlrs[t], (t, dlrs[t], hlrs[t])


@pytest.mark.parametrize("max_norm", [None, 1.0, 1e3])
def test_tail_equals_the_fp64_tail(max_norm):
    ps, grads = _main_case()
    ref_ps, ref_norms, ref_lrs, ref_coefs, _, _ = _main_ref(max_norm)
    if max_norm == 1.0:
        assert all(c < 1.0 for c in ref_coefs)                    # clipping active on every step
    if max_norm == 1e3:
        assert [c < 1.0 for c in ref_coefs] == [True] + [False] * 6      # ... on the first step only
    dev_ps, opt, sched = _build(ps, max_norm, 3)
    norms, dlrs, hlrs = _steps(dev_ps, opt, sched, grads)
    _check_norms_and_lrs(norms, dlrs, hlrs, ref_norms, max_norm is not None)
    assert hlrs == pytest.approx(ref_lrs, rel=1e-15)              # the host mirror is the schedule of the fp64 tail
    _close(dev_ps, ref_ps)
    assert float(opt.state[dev_ps[0]]["step"]) == 7.0 and sched.last_epoch == 7


def test_tail_is_bitwise_reproducible():
    ps, grads = _main_case()
    runs = []
    for _ in range(2):
        dev_ps, opt, sched = _build(ps, 1.0, 3)
        norms, _, _ = _steps(dev_ps, opt, sched, grads[:3])
        runs.append((norms, dev_ps))
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b)


def test_tail_without_clip_or_schedule_is_the_old_entry_point_bit_for_bit():
    """max_grad_norm = 1e30 makes coef exactly 1 and routes step() to rqhip_adamw_tail_step; no schedule: the lr is the argument."""
    from rqhip.optim import FlatAdamW
    ps, grads = _main_case()
    out = []
    for max_norm in (None, 1e30):
        dev_ps = [p.cuda().requires_grad_(True) for p in ps]
        opt = FlatAdamW(dev_ps, lr=LR, weight_decay=WD, max_grad_norm=max_norm)
        for gs in grads[:3]:
            _set_grads(dev_ps, gs)
            opt.step()
        out.append((dev_ps, [opt.state[p]["exp_avg"] for p in dev_ps], [opt.state[p]["exp_avg_sq"] for p in dev_ps]))
        if max_norm is not None:
            assert float(opt._tail[0][0][3]) == 1.0 and float(opt.device_lr(0)) == float(torch.tensor(LR, dtype=torch.float32))
        else:
            assert not opt._tail                  # the old entry point ran: no tail state was ever made
    for old, new in zip(out[0], out[1]):
        for a, b in zip(old, new):
            assert torch.equal(a, b)


def test_tail_on_thirty_odd_tensors_with_a_missing_and_a_misaligned_gradient():
    """30 tensors cross the 24-job boundary of the old launch; numels around the 1024-element workgroup and the float4 tail."""
    ps, grads, (ref_ps, ref_norms, ref_lrs, ref_coefs, _, _) = _odd_case()
    assert all(c < 1.0 for c in ref_coefs)
    dev_ps, opt, sched = _build(ps, 1.0, 2)
    norms, dlrs, hlrs = _steps(dev_ps, opt, sched, grads, misaligned=(ODD_MISALIGNED,))
    _check_norms_and_lrs(norms, dlrs, hlrs, ref_norms, True)
    _close(dev_ps, ref_ps)
    assert torch.equal(dev_ps[ODD_NONE].detach().cpu(), ps[ODD_NONE])           # no gradient: untouched, and not in the norm
    assert dev_ps[ODD_NONE] not in opt.state or "exp_avg" not in opt.state[dev_ps[ODD_NONE]]
    # and again: the same bits
    dev2, opt2, sched2 = _build(ps, 1.0, 2)
    norms2, _, _ = _steps(dev2, opt2, sched2, grads, misaligned=(ODD_MISALIGNED,))
    assert norms == norms2 and all(torch.equal(a, b) for a, b in zip(dev_ps, dev2))


def test_tail_in_a_captured_graph_crosses_the_warmup_boundary():
    """The pattern of tests/test_gpu_optim.py:test_flat_adamw_in_a_captured_graph_advances_its_step_counter."""
    import numpy as np
    g = torch.Generator().manual_seed(3)
    ps = [torch.randn(s, generator=g) for s in SHAPES]
    static = [torch.randn(s, generator=g) for s in SHAPES]
    dev_ps, opt, sched = _build(ps, 1.0, 2, wd=0.0)
    static_g = [x.cuda() for x in static]
    for p, x in zip(dev_ps, static_g):
        p.grad = x
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        opt.step()
    torch.cuda.current_stream().wait_stream(s)
    sched.step()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    for _ in range(4):
        graph.replay()
        sched.step()
    torch.cuda.synchronize()
    assert float(opt.state[dev_ps[0]]["step"]) == 5.0           # one eager step + four replays (the capture executes nothing)
    assert int(opt.device_lr_step(0)) == 6 == sched.last_epoch + 1
    want = LR * math.sqrt(2.0) / math.sqrt(5.0)                 # the lr of step 5: past the warm-up, which no captured argument reaches
    assert abs(float(opt.device_lr(0)) - float(np.float32(want))) <= ULP * want
    ref_ps, ref_norms, _, _, _, _ = _ref_tail(ps, [static] * 5, 1.0, 2, wd=0.0)
    assert abs(float(opt.grad_norm) - ref_norms[-1]) <= NORM_RTOL * ref_norms[-1]
    _close(dev_ps, ref_ps)


def test_tail_resumes_bit_for_bit_from_its_state_dicts():
    ps, grads = _main_case()
    whole_ps, opt, sched = _build(ps, 1.0, 3)
    _steps(whole_ps, opt, sched, grads[:6])
    a_ps, a_opt, a_sched = _build(ps, 1.0, 3)
    _steps(a_ps, a_opt, a_sched, grads[:3])
    osd, ssd = a_opt.state_dict(), a_sched.state_dict()
    assert set(osd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and "max_grad_norm" not in osd["param_groups"][0]
    b_ps, b_opt, b_sched = _build([p.detach().cpu() for p in a_ps], 1.0, 3)
    b_opt.load_state_dict(osd)
    b_sched.load_state_dict(ssd)
    norms, dlrs, hlrs = _steps(b_ps, b_opt, b_sched, grads[3:6])
    _check_norms_and_lrs(norms, dlrs, hlrs, _main_ref(1.0)[1][3:6], True)
    for a, b in zip(whole_ps, b_ps):
        assert torch.equal(a, b)
    assert float(b_opt.state[b_ps[0]]["step"]) == 6.0


def test_tail_continues_from_a_torch_adamw_checkpoint():
    from modules.scheduler.inv_sqrt import InverseSquareRootScheduler
    ps, grads = _main_case()
    t_ps = [p.cuda().requires_grad_(True) for p in ps]
    t_opt = torch.optim.AdamW(t_ps, lr=LR, weight_decay=WD, foreach=True)
    t_sched = InverseSquareRootScheduler(optimizer=t_opt, warmup_steps=3)
    for gs in grads[:3]:
        _set_grads(t_ps, gs)
        torch.nn.utils.clip_grad_norm_(t_ps, 1.0)
        t_opt.step()
        t_sched.step()
    b_ps, b_opt, b_sched = _build([p.detach().cpu() for p in t_ps], 1.0, 3)
    b_opt.load_state_dict(t_opt.state_dict())
    b_sched.load_state_dict(t_sched.state_dict())
    _steps(b_ps, b_opt, b_sched, grads[3:6])
    ref_ps = _ref_tail(ps, grads[:6], 1.0, 3)[0]
    _close(b_ps, ref_ps)
    assert float(b_opt.state[b_ps[0]]["step"]) == 6.0 and b_sched.last_epoch == 6


def test_tail_on_the_retrieval_model_s_parameter_list():
    """Against clip_grad_norm_ + torch.optim.AdamW(foreach) + the scheduler on a deep copy fed the same gradients: the tied shared /
    embed_tokens table, the decoder's never-used embed_tokens (.grad None), bos_token and sep_token."""
    from modules.model import EncoderDecoderRetrievalModel
    from modules.scheduler.inv_sqrt import InverseSquareRootScheduler
    from rqhip.optim import FlatAdamW
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(11)
    B, items, L, K, N = 4, 3, 3, 8, 20
    corpus = torch.randint(0, K, (N, L), generator=g)
    batch = to_device(synthetic_batch(corpus, B, items, g), dev)
    torch.manual_seed(11)
    a = EncoderDecoderRetrievalModel(corpus, L, K, t5_d_model=64, t5_num_heads=2, t5_d_ff=128, t5_num_layers=1).to(dev)
    a.attention_impl = a.norm_impl = a.head_impl = a.ffn_impl = "torch"
    a.eval()
    b = copy.deepcopy(a)
    a_opt = FlatAdamW(a.parameters(), lr=1e-3, weight_decay=WD, max_grad_norm=1.0)
    a_sched = InverseSquareRootScheduler(optimizer=a_opt, warmup_steps=1)
    b_opt = torch.optim.AdamW(b.parameters(), lr=1e-3, weight_decay=WD, foreach=True)
    b_sched = InverseSquareRootScheduler(optimizer=b_opt, warmup_steps=1)
    a_list, b_list = list(a.parameters()), list(b.parameters())
    assert len(a_list) == len(b_list)
    for _ in range(2):
        a.zero_grad(set_to_none=True)
        a(batch).loss.backward()
        assert any(p.grad is None for p in a_list) and any(p.grad is not None for p in a_list)
        for pa, pb in zip(a_list, b_list):
            pb.grad = None if pa.grad is None else pa.grad.clone()
        a_opt.step()
        a_sched.step()
        norm64 = math.sqrt(sum(float((p.grad.double() ** 2).sum()) for p in b_list if p.grad is not None))
        torch.nn.utils.clip_grad_norm_(b_list, 1.0)
        b_opt.step()
        b_sched.step()
        assert abs(float(a_opt.grad_norm) - norm64) <= NORM_RTOL * norm64
    assert a_opt.param_groups[0]["lr"] == b_opt.param_groups[0]["lr"]
    for (name, pa), pb in zip(a.named_parameters(), b_list):
        err, bound = (pa - pb).abs().max().item(), 1e-6 * max(1.0, pb.abs().max().item())
        assert err <= bound, (name, err, bound)
