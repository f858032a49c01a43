"""The host half of the retrieval loop's optimizer tail (reference train_decoder.py:147-151, 202-205), no GPU:
modules/scheduler/inv_sqrt.py:InverseSquareRootScheduler against values recorded from the reference's class
(tests/golden/inv_sqrt_sched.npz, written by tools/gen_retrieval_golden.py:gen_inv_sqrt_sched), the argument checks of
rqhip_adamw_tail_step / rqhip_adamw_tail_workspace_bytes (made before any HIP call), and FlatAdamW's refusal to clip across
param groups."""
import ctypes as C

import pytest
import torch

from conftest import load_golden

CASES = ("w3", "w1")


def _loop(warmup, base_lr, steps, sched=None, opt=None, p=None):
    """optimizer.step(), then scheduler.step(): the reference's loop -> (lr each optimizer step ran at, get_last_lr() after)."""
    from modules.scheduler.inv_sqrt import InverseSquareRootScheduler
    if sched is None:
        p = torch.nn.Parameter(torch.ones(3))
        opt = torch.optim.AdamW([p], lr=base_lr)
        sched = InverseSquareRootScheduler(optimizer=opt, warmup_steps=warmup)
    used, last = [], []
    for _ in range(steps):
        p.grad = torch.ones(3)
        used.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
        last.append(sched.get_last_lr()[0])
    return used, last, sched, opt, p


@pytest.mark.parametrize("case", CASES)
def test_scheduler_lr_sequence_equals_the_reference(case):
    g = load_golden("inv_sqrt_sched.npz")
    base_lr, warmup, steps = g[f"{case}.config"]
    used, last, sched, _, _ = _loop(int(warmup), float(base_lr), int(steps))
    assert used == [float(x) for x in g[f"{case}.lr_used"]]          # equal as Python floats, not close
    assert last == [float(x) for x in g[f"{case}.last_lr"]]
    # the closed form of the module's docstring: lr of optimizer step t
    W = int(warmup)
    for t, lr in enumerate(used, start=1):
        assert lr == (base_lr if t <= W else base_lr * (W ** 0.5 / t ** 0.5))
    assert sched.last_epoch == int(steps)


def test_scheduler_state_dict_keys_are_the_reference_s():
    from modules.scheduler.inv_sqrt import InverseSquareRootScheduler
    g = load_golden("inv_sqrt_sched.npz")
    p = torch.nn.Parameter(torch.ones(3))
    sched = InverseSquareRootScheduler(torch.optim.AdamW([p], lr=1e-3), warmup_steps=3)
    assert sorted(sched.state_dict()) == [str(k) for k in g["state_dict_keys"]]
    assert "optimizer" not in sched.state_dict() and sched.state_dict()["warmup_steps"] == 3


@pytest.mark.parametrize("case", CASES)
def test_scheduler_save_load_continue(case):
    from modules.scheduler.inv_sqrt import InverseSquareRootScheduler
    g = load_golden("inv_sqrt_sched.npz")
    base_lr, warmup, steps = g[f"{case}.config"]
    used, last, sched, opt, _ = _loop(int(warmup), float(base_lr), 4)
    sd, osd = sched.state_dict(), opt.state_dict()
    assert [sd["last_epoch"], sd["_step_count"]] == [int(x) for x in g[f"{case}.after4"]]
    # a fresh pair built as train_decoder.py builds it (base lr, default last_epoch), then both states loaded
    p2 = torch.nn.Parameter(torch.ones(3))
    opt2 = torch.optim.AdamW([p2], lr=float(base_lr))
    sched2 = InverseSquareRootScheduler(optimizer=opt2, warmup_steps=int(warmup))
    opt2.load_state_dict(osd)
    sched2.load_state_dict(sd)
    used2, last2, _, _, _ = _loop(int(warmup), float(base_lr), int(steps) - 4, sched2, opt2, p2)
    assert used + used2 == [float(x) for x in g[f"{case}.lr_used"]]
    assert last + last2 == [float(x) for x in g[f"{case}.last_lr"]]


def test_tail_workspace_query_without_gpu():
    from rqhip import _lib
    l = _lib.lib()

    def ask(numel):
        arr = (C.c_int64 * max(len(numel), 1))(*numel)
        return l.rqhip_adamw_tail_workspace_bytes(arr, len(numel))
    # one fp32 partial per 1024-element workgroup of every tensor
    assert ask([1]) == 4
    assert ask([1024, 1025]) == 4 * (1 + 2)
    assert ask([]) == 0
    assert l.rqhip_adamw_tail_workspace_bytes(None, 0) == 0
    assert ask([0, 7]) == 4
    assert l.rqhip_adamw_tail_workspace_bytes(None, 2) == -1
    assert l.rqhip_adamw_tail_workspace_bytes(None, -1) == -1
    assert ask([5, -1]) == -1
    assert b"negative numel" in l.rqhip_last_error()


def test_tail_step_argument_checks_without_gpu():
    """Every one of these returns before the first HIP call (there is no device in this process)."""
    from rqhip import _lib
    l = _lib.lib()
    host = (C.c_float * 64)()                      # host memory stands in for device pointers: nothing dereferences it
    base = C.addressof(host)
    base += (-base) % 16
    one = (C.c_void_p * 1)(base)
    off4 = (C.c_void_p * 1)(base + 4)
    null1 = (C.c_void_p * 1)(None)
    n8 = (C.c_int64 * 1)(8)
    neg = (C.c_int64 * 1)(-8)
    step, lr_step, scalars, ws = base + 64, base + 72, base + 96, base + 128

    def call(p=one, g=one, m=one, v=one, numel=n8, n=1, step=step, lr_step=lr_step, scalars=scalars, ws=ws, ws_bytes=4,
             max_norm=1.0, warmup=3):
        return l.rqhip_adamw_tail_step(p, g, m, v, numel, n, step, lr_step, scalars, ws, ws_bytes, max_norm, 1e-3, 1e-3, warmup,
                                       0.9, 0.999, 1e-8, 1e-2, None)
    E = _lib.EARG
    assert call(n=-1) == E and b"negative count" in l.rqhip_last_error()
    assert call(p=None) == E and call(g=None) == E and call(m=None) == E and call(v=None) == E and call(numel=None) == E
    assert call(step=None) == E and call(scalars=None) == E
    assert b"null pointer" in l.rqhip_last_error()
    assert call(scalars=scalars + 4) == E and b"aligned" in l.rqhip_last_error()
    assert call(lr_step=lr_step + 4) == E
    assert call(lr_step=None) == E and b"needs lr_step" in l.rqhip_last_error()      # a schedule without its counter
    assert call(numel=neg) == E and b"negative numel" in l.rqhip_last_error()
    assert call(g=off4) == E and b"tensor 0" in l.rqhip_last_error()                 # a misaligned gradient
    assert call(p=off4) == E and call(m=off4) == E and call(v=off4) == E
    assert call(m=null1) == E and b"tensor 0" in l.rqhip_last_error()
    assert call(ws=None) == E and b"workspace" in l.rqhip_last_error()               # clipping needs its partials
    assert call(ws_bytes=0) == E
    assert call(ws=ws + 2) == E


def test_flat_adamw_keeps_clipping_out_of_param_groups_and_refuses_two_groups():
    """The norm is global and the reference has one group: FlatAdamW(max_grad_norm=...) with two param groups raises at step()
    (not at construction: max_grad_norm is a settable attribute and add_param_group() can come later) -- before anything is launched,
    so the check runs without a GPU."""
    from rqhip.optim import FlatAdamW
    a, b = torch.nn.Parameter(torch.ones(4)), torch.nn.Parameter(torch.ones(4))
    opt = FlatAdamW([{"params": [a]}, {"params": [b]}], lr=1e-3, max_grad_norm=1.0)
    assert opt.max_grad_norm == 1.0
    assert all("max_grad_norm" not in g for g in opt.param_groups)
    assert "max_grad_norm" not in opt.state_dict()["param_groups"][0] and set(opt.state_dict()) == {"state", "param_groups"}
    a.grad, b.grad = torch.ones(4), torch.ones(4)
    with pytest.raises(ValueError, match="one param group"):
        opt.step()
    opt.max_grad_norm = None                # settable: without clipping two groups are fine again (a host tensor still is not)
    from rqhip._lib import RqHipError
    with pytest.raises(RqHipError, match="ROCm device parameters"):
        opt.step()
    one = FlatAdamW([a], lr=1e-3, max_grad_norm=-1.0)
    with pytest.raises(ValueError, match="positive"):
        one.step()
