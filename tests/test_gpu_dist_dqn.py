"""C51Policy / QRDQNPolicy on the device path (tianshou_amd/policy/c51.py, qrdqn.py,
dqn_dist.py, csrc/dqn_dist.hip).

Kernels: against an f64 restatement of the reference lines (c51.py:71-102, qrdqn.py:73-93) on
the same f32 inputs, at b in {1, 63, 64, 65, 257} x A in {1, 2, 6, 18} x N in {2, 51, 64, 65,
200} (the wave boundary, a non-multiple of 64, both default N).  tsrl_dist_select: q within
2 ulp of the f64 value rounded to f32; act the f64 argmax on every row whose f64 top-two
relative gap is >= 1e-6 (tests/test_dist_dqn_host.py shows on the CPU that the seeds below
exclude at most 1 % of any case's rows that way); row_out an exact copy.  Both losses, the
tolerances of test_gpu_dqn.py's test_td_fwd_bwd_matches_torch against f64: loss rtol 1e-5,
per-row vector (cross-entropy / priority) rtol 1e-5, gradient rtol 1e-4, each with atol 1e-6 *
max|ref|.  The torch fp32 formulation runs beside the kernel and its own deviation from f64 is
printed; the kernels sum in f64, so they are held to the bounds above at every shape and the
4 x torch allowance is not needed.  Measured on an MI355X over all 100 shapes, weighted and
not, as a fraction of max|ref|: C51 kernel loss 5.5e-8, ce 5.4e-8, gradient 5.5e-8 (torch fp32
1.7e-7, 2.4e-7, 2.6e-7); QR kernel loss 5.1e-8, prio 5.8e-8, gradient 4.9e-8 (torch fp32
1.6e-7, 1.7e-7, 2.1e-7); tsrl_dist_select's q 0 ulp from the rounded f64 value, no row excluded.

update() against tests/golden/dist_dqn.npz (tools/gen_goldens.py gen_dist_dqn;
tests/test_dist_dqn_host.py pins that file): sampled indices equal, returns rtol 1e-5 (with
test_gpu_dqn.py's atol 1e-6: a QR-DQN return r + gamma^n theta near zero carries the absolute
error of the GPU GEMM behind theta, about 1e-7 of its summands, which no rtol covers), losses
rtol 2e-5, outgoing weights rtol 1e-4, Adam parameters
rtol 1e-5 / atol 1e-6, tree leaves and priorities rtol 1e-4, and the importance weights of
the next sample rtol 1e-4 (a weight is (leaf / min leaf)^-0.4: two leaves inside 1e-4 each
move it by at most 0.4 * 2e-4).  With RMSprop the parameter bound is 4 x what ``fused = False``
(torch autograd + torch.optim.RMSprop) deviates from the same recording in the same test
(measured max |parameter - recorded|: torch 4.47e-8 after every update, fused 2.98e-8, 5.96e-8,
5.59e-8, 5.96e-8, 5.96e-8, 5.96e-8; the Adam variants at most 1.12e-7, fused and torch)."""
import json
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tianshou_amd import _C
from tianshou_amd.policy import C51Policy, QRDQNPolicy
from tianshou_amd.policy import dqn as dqn_mod
from tianshou_amd.policy.dqn_dist import _C51Loss, _QRLoss, dist_select

pytestmark = pytest.mark.gpu

for _name in ("tsrl_dist_select", "tsrl_c51_loss_fwd_bwd", "tsrl_qr_loss_fwd_bwd"):
    assert _name in _C.EXPORTED

BS = (1, 63, 64, 65, 257)
AS = (1, 2, 6, 18)
NS = (2, 51, 64, 65, 200)
V_MIN, V_MAX = -10.0, 10.0


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "dist_dqn.npz"))


# -- tsrl_dist_select -------------------------------------------------------------------------------
def select_inputs(b, A, N, mode):
    """CPU tensors (sel, eval, w) of one case: "c51" probabilities with the support as
    weights, "qr" plain values reduced by their mean."""
    g = torch.Generator().manual_seed(100000 * b + 1000 * A + N + (7 if mode == "qr" else 0))
    sel = torch.randn(b, A, N, generator=g)
    ev = torch.randn(b, A, N, generator=g)
    if mode == "c51":
        return sel.softmax(-1), ev.softmax(-1), torch.linspace(V_MIN, V_MAX, N)
    return sel, ev, None


def q_f64(sel, w):
    s = sel.double()
    return (s * w.double()).sum(2) if w is not None else s.mean(2)


def top2_rel_gap(q64):
    """Per row (best - second) / max(|best|, |second|) of an f64 [b, A] table; inf at A 1."""
    if q64.shape[1] < 2:
        return torch.full((q64.shape[0],), float("inf"), dtype=torch.float64)
    top = q64.topk(2, dim=1)[0]
    return (top[:, 0] - top[:, 1]) / top.abs().max(dim=1)[0]


def _ulp(x32):
    ax = x32.abs()
    return torch.nextafter(ax, torch.full_like(ax, float("inf"))) - ax


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("b", BS)
def test_dist_select_matches_f64(dev, b, A, N):
    for mode in ("c51", "qr"):
        sel, ev, w = select_inputs(b, A, N, mode)
        q64 = q_f64(sel, w)
        keep = (top2_rel_gap(q64) >= 1e-6).to(dev)
        act_ref = torch.as_tensor(q64.numpy().argmax(axis=1), device=dev)
        sel, ev = sel.to(dev), ev.to(dev)
        w = None if w is None else w.to(dev)
        q, act, row = dist_select(sel, ev, w, want_q=True, want_row=True)
        ref32 = q64.float().to(dev)
        worst = ((q - ref32).abs() / _ulp(ref32)).max().item()
        print(f"b {b} A {A} N {N} {mode}: q max {worst:.2f} ulp, rows kept "
              f"{int(keep.sum())}/{b}")
        assert worst <= 2.0
        assert act.dtype == torch.int64 and torch.equal(act[keep], act_ref[keep])
        rows = torch.arange(b, device=dev)
        assert torch.equal(row, ev[rows, act])
        # eval null: the row comes from sel; outputs not asked for are not written
        q2, act2, row2 = dist_select(sel, None, w, want_row=True)
        assert q2 is None and torch.equal(act2, act) and torch.equal(row2, sel[rows, act])
        q3, act3, row3 = dist_select(sel, ev, w, want_q=True, want_act=False)
        assert act3 is None and row3 is None and torch.equal(q3, q)


def test_dist_select_constructed_rows(dev):
    b, A, N = 70, 6, 65
    g = torch.Generator().manual_seed(5)
    sel = torch.randn(b, A, N, generator=g)
    sel[0:10, 4] = sel[0:10, 2] = sel[0:10, 1] + 1.0     # ties among the maxima: 2 before 4
    sel[0:10, 1] -= 3.0
    sel[10:20] = 0.25                                     # constant rows: action 0
    sel[20:30, 3, 7] = float("nan")                       # one NaN action beats every number
    sel[30:40, 5, 0] = sel[30:40, 2, 64] = float("nan")   # the first NaN wins
    sel[40:50, 0] = 50.0                                  # the maximum at the first action
    sel[50:60, 5] = 50.0                                  # and at the last (another wave's)
    ev = torch.randn(b, A, N, generator=g)
    sel, ev = sel.to(dev), ev.to(dev)
    rows = torch.arange(b, device=dev)
    for w in (None, torch.linspace(1.0, 2.0, N).to(dev)):  # positive weights keep the order
        q, act, row = dist_select(sel, ev, w, want_q=True, want_row=True)
        assert act[0:10].tolist() == [2] * 10
        assert torch.equal(q[0:10, 2], q[0:10, 4])
        assert act[10:20].tolist() == [0] * 10
        assert act[20:30].tolist() == [3] * 10 and bool(q[20:30, 3].isnan().all())
        assert act[30:40].tolist() == [2] * 10
        assert act[40:50].tolist() == [0] * 10 and act[50:60].tolist() == [5] * 10
        assert torch.equal(row, ev[rows, act])
    # A = 1: the only action, whatever its value
    one = torch.full((3, 1, N), float("-inf"), device=dev)
    assert dist_select(one)[1].tolist() == [0, 0, 0]
    # b = 0 launches nothing
    q, act, row = dist_select(sel[:0], None, None, want_q=True, want_row=True)
    assert q.shape == (0, A) and act.shape == (0,) and row.shape == (0, N)


# -- C51 loss ---------------------------------------------------------------------------------------
def c51_reference(curr, act, nxt, returns, support, weight, v_min, v_max, delta_z):
    """c51.py:82-102 in the dtype of ``curr``; returns (loss, ce, d loss / d curr)."""
    curr = curr.detach().clone().requires_grad_(True)
    tz = returns.clamp(v_min, v_max)
    target = ((1 - (tz.unsqueeze(1) - support.view(1, -1, 1)).abs() / delta_z).clamp(0, 1)
              * nxt.unsqueeze(1)).sum(-1)
    ca = curr[torch.arange(len(act), device=curr.device), act, :]
    ce = -(target * torch.log(ca + 1e-8)).sum(1)
    loss = (ce * (1.0 if weight is None else weight)).mean()
    loss.backward()
    return loss.detach(), ce.detach(), curr.grad


def _f64(*ts):
    return tuple(None if t is None else (t.double() if t.is_floating_point() else t)
                 for t in ts)


def c51_inputs(b, A, N, dev, weighted):
    g = torch.Generator().manual_seed(31 * b + 7 * A + N + int(weighted))
    curr = torch.randn(b, A, N, generator=g).softmax(-1)
    act = torch.randint(0, A, (b,), generator=g)
    nxt = torch.randn(b, N, generator=g).softmax(-1)
    support = torch.linspace(V_MIN, V_MAX, N)
    # r + gamma z with r ~ N(0, 3): both ends of the support clamp some returns
    returns = 3.0 * torch.randn(b, 1, generator=g) + 0.97 * support
    weight = torch.rand(b, generator=g) + 0.1 if weighted else None
    d = lambda t: None if t is None else t.to(dev).contiguous()  # noqa: E731
    return d(curr), d(act), d(nxt), d(returns), d(support), d(weight)


def _c51_kernel(curr, act, nxt, returns, support, weight, v_min=V_MIN, v_max=V_MAX):
    delta_z = (v_max - v_min) / (support.numel() - 1)
    x = curr.clone().requires_grad_(True)
    loss, ce = _C51Loss.apply(x, (act, nxt, returns, support, weight, v_min, v_max, delta_z,
                                  None, None))
    loss.backward()
    return loss.detach().clone(), ce.clone(), x.grad.clone()


def _dev_of(got, ref64):
    """max |got - ref| / (rtol-free scale max|ref|), for the printed figures."""
    scale = float(ref64.abs().max()) or 1.0
    return float((got.double() - ref64).abs().max()) / scale


def _assert_loss_outputs(got, ref64, what):
    """loss rtol 1e-5, per-row vector rtol 1e-5, gradient rtol 1e-4; atol 1e-6 max|ref|."""
    for (g, r, rtol, name) in zip(got, ref64, (1e-5, 1e-5, 1e-4), ("loss", "vec", "grad")):
        atol = 1e-6 * float(r.abs().max())
        torch.testing.assert_close(g.double(), r, rtol=rtol, atol=atol, msg=lambda m: f"{what} "
                                   f"{name}: {m}")


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("b", BS)
def test_c51_loss_matches_f64(dev, b, A, N):
    delta_z = (V_MAX - V_MIN) / (N - 1)
    for weighted in (False, True):
        args = c51_inputs(b, A, N, dev, weighted)
        curr, act, nxt, returns, support, weight = args
        assert bool((returns < V_MIN).any()) and bool((returns > V_MAX).any()) or b < 63
        ref = c51_reference(*_f64(*args), V_MIN, V_MAX, delta_z)
        f32 = c51_reference(*args, V_MIN, V_MAX, delta_z)
        got = _c51_kernel(*args)
        print(f"b {b} A {A} N {N} w {int(weighted)}: kernel / torch-f32 deviation from f64, "
              "over max|ref|: " + ", ".join(
                  f"{n} {_dev_of(k, r):.2e} / {_dev_of(t, r):.2e}"
                  for n, k, t, r in zip(("loss", "ce", "grad"), got, f32, ref)))
        _assert_loss_outputs(got, ref, f"c51 b {b} A {A} N {N}")
        loss, ce, grad = got
        off = torch.ones_like(grad, dtype=torch.bool)
        off[torch.arange(b, device=dev), act] = False
        assert (grad[off] == 0).all()
        for a, c in zip(got, _c51_kernel(*args)):  # a fixed summation order
            assert torch.equal(a, c)
        # next sums to 1, so does the projected target the gradient implies
        w = torch.ones(b, device=dev) if weight is None else weight
        ga = grad[torch.arange(b, device=dev), act].double()
        ca = curr[torch.arange(b, device=dev), act].double()
        implied = (-ga * (ca + 1e-8) * b / w.double().unsqueeze(1)).sum(1)
        torch.testing.assert_close(implied, torch.ones_like(implied), rtol=0, atol=1e-5)


def test_c51_loss_constructed_rows(dev):
    b, A, N = 6, 3, 21
    v_min, v_max = -4.0, 4.0
    delta_z = (v_max - v_min) / (N - 1)
    g = torch.Generator().manual_seed(9)
    support = torch.linspace(v_min, v_max, N)
    curr = torch.randn(b, A, N, generator=g).softmax(-1)
    nxt = torch.randn(b, N, generator=g).softmax(-1)
    act = torch.tensor([0, 1, 2, 0, 1, 2])
    returns = torch.empty(b, N)
    returns[0] = -4.5 - torch.rand(N, generator=g)   # all below v_min: all mass on atom 0
    returns[1] = 4.0 + torch.rand(N, generator=g)    # all at or above v_max: on atom N - 1
    returns[2] = support                             # exactly on the atoms: target = next
    returns[3] = 0.3                                 # a terminal row: one value between atoms
    returns[4] = 1.0 + 0.97 * support
    returns[5] = 1.0 + 0.97 * support
    curr[4, 1, 5] = 0.0                              # log(0 + 1e-8) stays finite
    args = tuple(t.to(dev).contiguous() for t in (curr, act, nxt, returns, support))
    for weight in (None, (torch.rand(b, generator=g) + 0.5).to(dev)):
        full = args + (weight,)
        ref = c51_reference(*_f64(*full), v_min, v_max, delta_z)
        got = _c51_kernel(*full, v_min=v_min, v_max=v_max)
        # the zero probability's gradient entry (~ -t / 1e-8) would hide every other entry
        # behind atol = 1e-6 max|ref|: compare the rows apart
        for r in range(b):
            _assert_loss_outputs((got[0], got[1][r:r + 1], got[2][r]),
                                 (ref[0], ref[1][r:r + 1], ref[2][r]), f"row {r}")
        loss, ce, grad = got
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
        w = torch.ones(b, device=dev) if weight is None else weight
        rows = torch.arange(b, device=dev)
        implied = -grad[rows, args[1]].double() * (args[0][rows, args[1]].double() + 1e-8) \
            * b / w.double().unsqueeze(1)
        one_hot = torch.zeros(N, dtype=torch.float64, device=dev)
        torch.testing.assert_close(implied[0], one_hot.index_fill(0, torch.tensor(0, device=dev),
                                                                  1.0), rtol=0, atol=1e-5)
        torch.testing.assert_close(implied[1], one_hot.index_fill(
            0, torch.tensor(N - 1, device=dev), 1.0), rtol=0, atol=1e-5)
        torch.testing.assert_close(implied[2], args[2][2].double(), rtol=0, atol=1e-5)
        # 0.3 lies between atoms 10 (0.0) and 11 (0.4): 1/4 and 3/4 of the mass
        want = one_hot.clone()
        want[10], want[11] = 0.25, 0.75
        torch.testing.assert_close(implied[3], want, rtol=0, atol=1e-5)
        torch.testing.assert_close(ce[0].double(), -torch.log(args[0][0, 0, 0].double() + 1e-8),
                                   rtol=1e-5, atol=0)
    # an invalid action: NaN loss and cross-entropy, a zero gradient row, the others as before
    for bad in (-1, A):
        act_bad = args[1].clone()
        act_bad[3] = bad
        loss_b, ce_b, grad_b = _c51_kernel(args[0], act_bad, *args[2:], None, v_min=v_min,
                                           v_max=v_max)
        good = _c51_kernel(*args, None, v_min=v_min, v_max=v_max)
        assert bool(loss_b.isnan()) and bool(ce_b[3].isnan())
        assert (grad_b[3] == 0).all()
        keep = torch.tensor([0, 1, 2, 4, 5], device=dev)
        assert torch.equal(grad_b[keep], good[2][keep]) and torch.equal(ce_b[keep], good[1][keep])


# -- QR loss ----------------------------------------------------------------------------------------
def qr_reference(curr, act, returns, tau_hat, weight):
    """qrdqn.py:82-93 in the dtype of ``curr``; returns (loss, prio, d loss / d curr)."""
    curr = curr.detach().clone().requires_grad_(True)
    b, _, N = curr.shape
    ca = curr[torch.arange(b, device=curr.device), act, :].unsqueeze(2)
    target = returns.unsqueeze(1)
    diff = F.smooth_l1_loss(target.expand(-1, N, -1), ca.expand(-1, -1, N), reduction="none")
    huber = (diff * (tau_hat.view(1, -1, 1) - (target - ca).detach().le(0.).to(curr.dtype))
             .abs()).sum(-1).mean(1)
    loss = (huber * (1.0 if weight is None else weight)).mean()
    prio = diff.detach().abs().sum(-1).mean(1)
    loss.backward()
    return loss.detach(), prio, curr.grad


def _tau_hat(N, dev):
    tau = torch.linspace(0, 1, N + 1)
    return ((tau[:-1] + tau[1:]) / 2).to(dev).contiguous()


def qr_inputs(b, A, N, dev, weighted):
    g = torch.Generator().manual_seed(17 * b + 5 * A + N + int(weighted))
    curr = torch.randn(b, A, N, generator=g)
    act = torch.randint(0, A, (b,), generator=g)
    returns = 2.0 * torch.randn(b, N, generator=g)  # |u| below and above the Huber knee
    weight = torch.rand(b, generator=g) + 0.1 if weighted else None
    d = lambda t: None if t is None else t.to(dev).contiguous()  # noqa: E731
    return d(curr), d(act), d(returns), _tau_hat(N, dev), d(weight)


def _qr_kernel(curr, act, returns, tau_hat, weight):
    x = curr.clone().requires_grad_(True)
    loss, prio = _QRLoss.apply(x, (act, returns, tau_hat, weight, None, None))
    loss.backward()
    return loss.detach().clone(), prio.clone(), x.grad.clone()


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("b", BS)
def test_qr_loss_matches_f64(dev, b, A, N):
    for weighted in (False, True):
        args = qr_inputs(b, A, N, dev, weighted)
        ref = qr_reference(*_f64(*args))
        f32 = qr_reference(*args)
        got = _qr_kernel(*args)
        print(f"b {b} A {A} N {N} w {int(weighted)}: kernel / torch-f32 deviation from f64, "
              "over max|ref|: " + ", ".join(
                  f"{n} {_dev_of(k, r):.2e} / {_dev_of(t, r):.2e}"
                  for n, k, t, r in zip(("loss", "prio", "grad"), got, f32, ref)))
        _assert_loss_outputs(got, ref, f"qr b {b} A {A} N {N}")
        grad = got[2]
        off = torch.ones_like(grad, dtype=torch.bool)
        off[torch.arange(b, device=dev), args[1]] = False
        assert (grad[off] == 0).all()
        for a, c in zip(got, _qr_kernel(*args)):
            assert torch.equal(a, c)


def test_qr_loss_constructed_pairs(dev):
    # N = 2, tau_hat = (1/4, 3/4); every u is exact in f32
    tau_hat = _tau_hat(2, dev)
    assert tau_hat.tolist() == [0.25, 0.75]
    curr = torch.tensor([[[0.0, 0.5], [9.0, 9.0]],       # u = (0, 1) and (-1/2, 1/2)
                         [[9.0, 9.0], [0.0, 0.0]],       # |u| >> 1: (100, -100) twice
                         [[1.0, -1.0], [9.0, 9.0]]],     # |u| == 1 on both sides, and 0
                        device=dev)
    act = torch.tensor([0, 1, 0], device=dev)
    returns = torch.tensor([[0.0, 1.0], [100.0, -100.0], [0.0, 0.0]], device=dev)
    loss, prio, grad = _qr_kernel(curr, act, returns, tau_hat, None)
    b, N = 3, 2
    # row 0, i = 0 (theta 0): u = (0, 1): h = (0, 1/2), k = (3/4, 1/4); the u == 0 pair adds
    # nothing to the gradient.  i = 1 (theta 1/2): u = (-1/2, 1/2): h = (1/8, 1/8), k = (1/4, 3/4)
    hub0 = (0.5 * 0.25 + 0.125 * 0.25 + 0.125 * 0.75) / N
    assert prio[0].item() == (0.5 + 0.125 + 0.125) / N
    f32 = lambda *xs: [float(np.float32(x)) for x in xs]  # noqa: E731
    assert grad[0, 0].tolist() == f32(-(1.0 * 0.25) / (b * N),
                                      -(-0.5 * 0.25 + 0.5 * 0.75) / (b * N))
    # row 1: h = |u| - 1/2 = 99.5, the gradient clamped to +-1
    hub1 = (99.5 * 0.25 + 99.5 * 0.75 + 99.5 * 0.75 + 99.5 * 0.25) / N
    assert prio[1].item() == 4 * 99.5 / N
    assert grad[1, 1].tolist() == f32(-(0.25 - 0.75) / (b * N), -(0.75 - 0.25) / (b * N))
    # row 2, i = 0 (theta 1): u = (-1, -1): h = 1/2, k = 3/4; i = 1 (theta -1): u = (1, 1),
    # k = 3/4: |u| == 1 sits on the quadratic and the linear branch alike
    hub2 = (0.5 * 0.75 * 2 + 0.5 * 0.75 * 2) / N
    assert prio[2].item() == 4 * 0.5 / N
    assert grad[2, 0].tolist() == f32(-(-2 * 0.75) / (b * N), -(2 * 0.75) / (b * N))
    np.testing.assert_allclose(loss.item(), (hub0 + hub1 + hub2) / b, rtol=1e-6)
    assert (grad[0, 1] == 0).all() and (grad[1, 0] == 0).all() and (grad[2, 1] == 0).all()
    ref = qr_reference(*_f64(curr, act, returns, tau_hat, None))
    _assert_loss_outputs((loss, prio, grad), ref, "constructed")
    # an invalid action
    act_bad = torch.tensor([0, 2, 0], device=dev)
    loss_b, prio_b, grad_b = _qr_kernel(curr, act_bad, returns, tau_hat, None)
    assert bool(loss_b.isnan()) and bool(prio_b[1].isnan()) and (grad_b[1] == 0).all()
    assert torch.equal(grad_b[0], grad[0]) and torch.equal(prio_b[[0, 2]], prio[[0, 2]])


# -- autograd wrappers --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("c51", "qr"))
def test_dist_loss_seed_paths(dev, kind):
    """Under the learn path's constant unit seed the backward hands the kernel's gradient over
    as it is; any other seed scales it; no seed at all gives no gradient."""
    from tianshou_amd.policy.onpolicy import _unit_seed
    if kind == "c51":
        curr, act, nxt, returns, support, weight = c51_inputs(257, 6, 51, dev, True)
        fn = _C51Loss
        args = (act, nxt, returns, support, weight, V_MIN, V_MAX, (V_MAX - V_MIN) / 50, None,
                None)
    else:
        curr, act, returns, tau_hat, weight = qr_inputs(257, 6, 51, dev, True)
        fn = _QRLoss
        args = (act, returns, tau_hat, weight, None, None)
    grads = []
    for seed in ("ones", "unit", 2.5):
        x = curr.clone().requires_grad_(True)
        loss, vec = fn.apply(x, args)
        assert not vec.requires_grad
        if seed == "ones":
            loss.backward()
        elif seed == "unit":
            loss.backward(_unit_seed(dev))
        else:
            (loss * seed).backward()
        grads.append(x.grad.clone())
    assert torch.equal(grads[0], grads[1])
    torch.testing.assert_close(grads[2], 2.5 * grads[0], rtol=1e-6, atol=0)

    class _Ctx:
        saved_tensors = (grads[0],)
        in_dtype = torch.float32
    assert fn.backward(_Ctx, None, None) == (None, None)
    # static outputs: the per-row vector lands in the buffer handed in, the loss in its own
    vec_out = torch.empty(257, device=dev)
    loss_out = torch.empty((), device=dev)
    loss, vec = fn.apply(curr.clone().requires_grad_(True), args[:-2] + (vec_out, loss_out))
    assert vec.data_ptr() == vec_out.data_ptr() and torch.equal(loss.detach(), loss_out)
    assert torch.equal(vec_out, fn.apply(curr, args)[1])


# -- update() against the recording -----------------------------------------------------------------
from tests import test_gpu_dqn as gd  # noqa: E402  (its buffer / recorder helpers)


def _cfg(z):
    return json.loads(str(z["learn_cfg"]))


def _policy(z, cfg, tag, dev, optim=None, **attrs):
    from tianshou_amd.utils.net import Net
    v = cfg["variants"][tag]
    kind = v["kind"]
    N = cfg["c51"]["num_atoms"] if kind == "c51" else cfg["qr"]["num_quantiles"]
    net = Net(cfg["D"], cfg["A"], hidden_sizes=tuple(cfg["hidden"]), device=dev,
              softmax=kind == "c51", num_atoms=N).to(dev)
    pre = f"init_{kind}_"
    net.load_state_dict({k[len(pre):]: torch.as_tensor(z[k]) for k in z.files
                         if k.startswith(pre)})
    if optim is None:
        optim = v["optim"]
    opt = {"rms": lambda p: torch.optim.RMSprop(p, lr=7e-4, eps=1e-5, alpha=0.99),
           "adam": lambda p: torch.optim.Adam(p, lr=1e-3),
           "sgd": lambda p: torch.optim.SGD(p, lr=1e-2)}[optim](net.parameters())
    kw = dict(discount_factor=cfg["gamma"], estimation_step=v["n_step"],
              target_update_freq=v["freq"])
    if kind == "c51":
        policy = C51Policy(net, opt, **cfg["c51"], **kw).to(dev)
    else:
        policy = QRDQNPolicy(net, opt, **cfg["qr"], **kw).to(dev)
    for k, a in attrs.items():
        setattr(policy, k, a)
    return policy, v


def _run_variant(z, dev, tag, check_params, **attrs):
    """Six update() calls of one recorded variant; everything but the parameters is asserted
    here, the parameters by ``check_params(u, policy)``."""
    cfg = _cfg(z)
    policy, v = _policy(z, cfg, tag, dev, **attrs)
    buf = gd._filled_buffer(z, cfg, dev, per=bool(v.get("per")))
    seen = gd._record(policy)
    np.random.seed(cfg["seed"])
    for u in range(6):
        res = policy.update(v["bs"], buf)
        q = f"{tag}_u{u}_"
        s = seen[u]
        assert s["indices"].tolist() == z[q + "indices"].tolist(), q
        out_w = s["td_error"]  # the recorder's name for the outgoing batch.weight
        print(f"{q} loss {res['loss']:.7g} recorded {float(z[q + 'loss']):.7g} "
              f"max|dparam| {gd._param_dev(policy.model, z, q + 'param_'):.3g} max rel dweight "
              f"{np.abs(out_w.cpu().numpy() / z[q + 'out_weight'] - 1).max():.3g} max|dreturns| "
              f"{np.abs(s['returns'].cpu().numpy() - z[q + 'returns']).max():.3g}")
        assert s["returns"].shape == z[q + "returns"].shape
        np.testing.assert_allclose(s["returns"].cpu().numpy(), z[q + "returns"], rtol=1e-5,
                                   atol=1e-6, err_msg=q)
        np.testing.assert_allclose(res["loss"], float(z[q + "loss"]), rtol=2e-5, err_msg=q)
        assert out_w.is_cuda and not out_w.requires_grad and out_w.shape == (v["bs"],)
        np.testing.assert_allclose(out_w.cpu().numpy(), z[q + "out_weight"], rtol=1e-4,
                                   err_msg=q)
        if v.get("per"):
            np.testing.assert_allclose(s["weight"].cpu().numpy(), z[q + "weight"], rtol=1e-4,
                                       err_msg=q)
            leaves = buf.weight[np.arange(buf.maxsize)]
            np.testing.assert_allclose(np.asarray(leaves), z[q + "leaves"], rtol=1e-4,
                                       err_msg=q)
        check_params(u, policy)
    if v.get("per"):
        np.testing.assert_allclose(buf._max_prio, float(z[tag + "_max_prio"]), rtol=1e-4)
        np.testing.assert_allclose(buf._min_prio, float(z[tag + "_min_prio"]), rtol=1e-4)
    assert policy._iter == 6
    return policy


# (variant, update after which model_old is looked at, update whose recorded parameters it holds)
SYNC_POINTS = {"c51_target": (3, 1), "qr_target": (4, 2)}


def _adam_check(z, tag):
    def check(u, policy):
        for k, t in policy.model.state_dict().items():
            np.testing.assert_allclose(t.cpu().numpy(), z[f"{tag}_u{u}_param_{k}"], rtol=1e-5,
                                       atol=1e-6, err_msg=f"{tag} update {u} {k}")
        if tag in SYNC_POINTS and u == SYNC_POINTS[tag][0]:
            # freq 2: the sync at _iter 2 copied the parameters recorded after update 1 and
            # update 3 left them alone; freq 3: _iter 3, update 2, update 4
            for k, t in policy.model_old.state_dict().items():
                np.testing.assert_allclose(t.cpu().numpy(),
                                           z[f"{tag}_u{SYNC_POINTS[tag][1]}_param_{k}"],
                                           rtol=1e-5, atol=1e-6, err_msg=f"model_old {k}")
            assert not any(torch.equal(a, b) for a, b in zip(policy.model.parameters(),
                                                             policy.model_old.parameters()))
    return check


ADAM_TAGS = ("c51_target", "c51_notarget", "c51_per", "qr_target", "qr_notarget", "qr_per")


@pytest.mark.parametrize("tag", ADAM_TAGS)
def test_update_matches_reference_adam(z, dev, tag):
    policy = _run_variant(z, dev, tag, _adam_check(z, tag))
    assert policy._flat is not None and policy._flat.adam_bound(policy.optim)
    assert policy._learn_graphs and not policy._graph_failed  # these updates replay


def test_update_matches_reference_rmsprop(z, dev):
    """The fused path's max |parameter - recorded| after each update stays within 4 x the
    torch formulation's on the same GPU (both printed)."""
    torch_dev = []
    _run_variant(z, dev, "qr_rms", lambda u, p: torch_dev.append(
        gd._param_dev(p.model, z, f"qr_rms_u{u}_param_")), fused=False)
    fused_dev = []

    def check(u, policy):
        fused_dev.append(gd._param_dev(policy.model, z, f"qr_rms_u{u}_param_"))
    policy = _run_variant(z, dev, "qr_rms", check)
    print("qr_rms max|dparam| per update: torch", torch_dev, "fused", fused_dev)
    assert policy._flat.adam_bound(policy.optim)
    assert set(policy.optim.state[next(policy.model.parameters())]) == {"step", "square_avg"}
    for u in range(6):
        assert fused_dev[u] <= 4 * torch_dev[u], (u, fused_dev[u], torch_dev[u])


@pytest.mark.parametrize("tag", ("c51_target", "c51_per", "qr_target", "qr_per"))
def test_torch_formulation_matches_reference(z, dev, tag):
    policy = _run_variant(z, dev, tag, _adam_check(z, tag), fused=False)
    assert policy._flat is None and not policy._learn_graphs


# -- paths taken ------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ("c51_target", "qr_target"))
def test_flat_storage_is_bound_with_plain_adam(z, dev, tag):
    cfg = _cfg(z)
    policy, v = _policy(z, cfg, tag, dev)
    buf = gd._filled_buffer(z, cfg, dev)
    np.random.seed(3)
    policy.update(v["bs"], buf)
    fa = policy._flat
    assert fa is not None and fa.adam_bound(policy.optim)
    flat = fa.flat_param
    lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * 4
    for p in policy.model.parameters():
        assert lo <= p.data_ptr() < hi
    # the support / tau_hat belong to the policy, not to the optimiser's flat storage
    own = policy.support if tag == "c51_target" else policy.tau_hat
    assert own.is_cuda and not lo <= own.data_ptr() < hi
    old = policy._old_flat
    assert old is not None and old.shape == flat.shape
    policy.update(v["bs"], buf)
    assert not torch.equal(old, flat)
    policy.sync_weight()
    assert torch.equal(old, flat)


@pytest.mark.parametrize("tag", ("c51_target", "qr_target"))
def test_other_optimisers_keep_torch_step(z, dev, tag):
    cfg = _cfg(z)
    policy, v = _policy(z, cfg, tag, dev, optim="sgd")
    buf = gd._filled_buffer(z, cfg, dev)
    before = [p.detach().clone() for p in policy.model.parameters()]
    np.random.seed(3)
    losses = [policy.update(v["bs"], buf)["loss"] for _ in range(3)]
    assert policy._flat is None or not policy._flat.adam_bound(policy.optim)
    assert not policy._learn_graphs
    assert all(np.isfinite(losses)) and len(set(losses)) == 3
    assert all(not torch.equal(a, b) for a, b in zip(before, policy.model.parameters()))


def _six_updates(z, dev, tag, sizes, **attrs):
    cfg = _cfg(z)
    policy, v = _policy(z, cfg, tag, dev, **attrs)
    buf = gd._filled_buffer(z, cfg, dev, per=bool(v.get("per")))
    np.random.seed(cfg["seed"])
    out = []
    for bs in sizes:
        loss = policy.update(bs, buf)["loss"]
        out.append((loss, [p.detach().clone() for p in policy.model.parameters()]))
    return policy, out


def _same_bits(out_g, out_e):
    for (loss_g, par_g), (loss_e, par_e) in zip(out_g, out_e):
        assert loss_g == loss_e
        for a, b in zip(par_g, par_e):
            assert torch.equal(a, b)


@pytest.mark.parametrize("tag", ("c51_target", "c51_per", "qr_target", "qr_per"))
def test_graph_replay_is_bitwise_eager(z, dev, tag):
    bs = _cfg(z)["variants"][tag]["bs"]
    pol_g, out_g = _six_updates(z, dev, tag, [bs] * 6, graph_learn=True)
    pol_e, out_e = _six_updates(z, dev, tag, [bs] * 6, graph_learn=False)
    assert len(pol_g._learn_graphs) == 1 and not pol_e._learn_graphs
    _same_bits(out_g, out_e)


@pytest.mark.parametrize("tag", ("c51_target", "qr_target"))
def test_graph_replay_follows_batch_size(z, dev, tag):
    sizes = [64, 64, 32, 64, 32, 32]
    pol_g, out_g = _six_updates(z, dev, tag, sizes, graph_learn=True)
    pol_e, out_e = _six_updates(z, dev, tag, sizes, graph_learn=False)
    assert sorted(k[0] for k in pol_g._learn_graphs) == [32, 64]
    _same_bits(out_g, out_e)


@pytest.mark.parametrize("tag", ("c51_target", "qr_target"))
def test_capture_failure_warns_once_and_stays_eager(z, dev, monkeypatch, tag):
    """A capture that raises RuntimeError (simulated on the host: the capture entry raises
    before torch.cuda.graph is entered, so no stream is ever capturing) warns once, latches
    _graph_failed and every update runs eagerly, still matching the recording."""
    tries = []

    def failing_capture(graph):
        tries.append(graph)
        raise RuntimeError("simulated capture failure")

    monkeypatch.setattr(dqn_mod, "graph_capture", failing_capture)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        policy = _run_variant(z, dev, tag, _adam_check(z, tag), graph_learn=True)
    msgs = [w for w in caught if "learn-graph capture failed" in str(w.message)]
    assert len(msgs) == 1 and len(tries) == 1
    assert policy._graph_failed and not policy._learn_graphs


# -- Collector --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("c51", "qr"))
def test_collect_greedy_fills_the_buffer(dev, kind):
    """eps 0: the stored actions are the argmax of the policy's own torch-formulation Q-values
    on the stored observations."""
    from tianshou_amd.data import Collector, VectorReplayBuffer
    from tianshou_amd.env import CartPoleEnv, Discrete, DummyVectorEnv
    from tianshou_amd.utils.net import Net
    E, n_step, size = 4, 120, 400
    envs = DummyVectorEnv([CartPoleEnv for _ in range(E)])
    np.random.seed(1627)
    torch.manual_seed(1627)
    envs.seed(1627)
    N = 51 if kind == "c51" else 200
    net = Net(4, 2, hidden_sizes=(16, 16), device=dev, softmax=kind == "c51",
              num_atoms=N).to(dev)
    optim = torch.optim.Adam(net.parameters(), lr=1e-3)
    policy = (C51Policy(net, optim, target_update_freq=10, action_space=Discrete(2))
              if kind == "c51" else
              QRDQNPolicy(net, optim, target_update_freq=10, action_space=Discrete(2))).to(dev)
    policy.set_eps(0.0)
    buf = VectorReplayBuffer(size, E, device=dev)
    col = Collector(policy, envs, buf, exploration_noise=True)
    res = col.collect(n_step=n_step)
    assert res["n/st"] == n_step and len(buf) == n_step
    steps, S = n_step // E, size // E
    m = buf._meta
    policy.fused = False
    with torch.no_grad():
        for t in range(steps):  # the collector's own batches: one row per env
            rows = torch.arange(E, device=dev) * S + t
            logits, _ = policy.model(m.obs[rows])
            assert logits.shape == (E, 2, N)
            q = policy.compute_q_value(logits, None)
            assert torch.equal(m.act[rows].reshape(-1), q.argmax(dim=1)), t
    policy.fused = True
    np.random.seed(4)
    losses = [policy.update(64, buf)["loss"] for _ in range(3)]
    assert all(np.isfinite(losses)) and len(set(losses)) == 3


# -- Atari heads ------------------------------------------------------------------------------------
def test_atari_heads(dev):
    from tianshou_amd.utils.net_atari import C51, DQN, QRDQN
    g = torch.Generator().manual_seed(2)
    obs = torch.randint(0, 256, (2, 4, 84, 84), generator=g, dtype=torch.uint8).to(dev)
    torch.manual_seed(0)
    A = 6
    c51 = C51(4, 84, 84, [A], num_atoms=51, device=dev).to(dev)
    with torch.no_grad():
        out, _ = c51(obs)
        trunk, _ = DQN.forward(c51, obs)
    assert trunk.shape == (2, A * 51) and out.shape == (2, A, 51)
    assert torch.equal(out, trunk.view(-1, 51).softmax(dim=-1).view(-1, A, 51))
    torch.testing.assert_close(out.sum(-1), torch.ones(2, A, device=dev), rtol=0, atol=1e-5)
    qr = QRDQN(4, 84, 84, [A], num_quantiles=200, device=dev).to(dev)
    with torch.no_grad():
        out, _ = qr(obs)
        trunk, _ = DQN.forward(qr, obs)
    assert out.shape == (2, A, 200) and torch.equal(out, trunk.view(2, A, 200))
    # the policies act on these outputs
    policy = C51Policy(c51, torch.optim.Adam(c51.parameters(), lr=1e-4)).to(dev)
    from tianshou_amd.data import Batch
    with torch.no_grad():
        act = policy(Batch(obs=obs, info=Batch())).act
    assert act.shape == (2,) and act.dtype == torch.int64
