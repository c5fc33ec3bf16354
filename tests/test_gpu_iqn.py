"""IQNPolicy / ImplicitQuantileNetwork on the device path (tianshou_amd/policy/iqn.py,
utils/net.py, the tsrl_iqn_* kernels of csrc/dqn_dist.hip).

Embed: tsrl_iqn_embed_fwd / _bwd against an f64 restatement of discrete.py:143-155, 211-212 on
the same f32 inputs (the cos argument formed in f32 as torch forms it, then everything in f64)
at B in {1, 3, 65} x N in {2, 8, 33} x D in {1, 64, 65, 200} x C in {1, 64, 65}, one Atari-width
case (2, 2, 3136, 64) and one at C = IQN_MAX_COSINES.  Every case holds a fraction of exactly 0
and the largest f32 below 1, and is run again with an all-zero W and bias (z == 0: e and g_z
exactly 0) and with one NaN in h (that row's outputs NaN, nothing else).  The torch f32
composition runs beside the kernel on the same inputs; the kernel may deviate from f64 by at
most 4 x what torch's leg deviates, both as a fraction of max|ref| (the allowance
test_gpu_dist_dqn.py names).  MEASURED_EMBED below holds the figures of an MI355X run.

Select and loss: against f64 restatements of qrdqn.py:58-73 and iqn.py:93-108 in both layouts
(contiguous [b, A, N] and the transposed view of [b, N, A]) with test_gpu_dist_dqn.py's bounds:
q within 2 ulp of the rounded f64 mean, act the f64 argmax wherever the f64 top-two relative gap
is >= 1e-6 (tests/test_iqn_host.py shows the seeds exclude at most 1 % of a case's rows), row an
exact copy; loss rtol 1e-5, priority rtol 1e-5, gradient rtol 1e-4, each with atol 1e-6 *
max|ref|.

update() against tests/golden/iqn.npz (tools/gen_goldens.py gen_iqn; tests/test_iqn_host.py
pins that file) with the recorded draws injected through ``_sample_taus``: indices equal,
returns rtol 1e-5 / atol 1e-6, losses rtol 2e-5, outgoing priorities rtol 1e-4, Adam parameters
rtol 1e-5 / atol 1e-6, RMSprop parameters within 4 x what ``fused = False`` deviates in the same
test."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tianshou_amd import _C
from tianshou_amd.policy import IQNPolicy
from tianshou_amd.policy.dqn_dist import _QRLoss
from tianshou_amd.policy.iqn import _IQNLoss, iqn_select
from tianshou_amd.utils.net import (CosineEmbeddingNetwork, ImplicitQuantileNetwork, Net,
                                    _IQNEmbedFn, _linear_grads)

pytestmark = pytest.mark.gpu

# max over all embed cases of the deviation from f64 as a fraction of max|ref|, kernel / torch
# f32, on an MI355X (printed per case by test_embed_matches_f64)
MEASURED_EMBED = """
e 5.4e-08 / 7.0e-07, out 5.9e-08 / 4.6e-07, g_h 1.5e-07 / 8.0e-07, g_W 1.7e-06 / 1.7e-06,
g_b 5.8e-08 / 8.6e-07, g_z 5.6e-08 / 5.6e-08; the largest kernel / torch ratio of any case and
output is 1.9 (g_W, the torch GEMM of both legs over cosine features that differ in the last
bit), every other output's is 1.0 or less.  The loss kernel over all of test_loss_matches_f64:
loss 5.4e-08 / 1.5e-07, priority 5.6e-08 / 1.8e-07, gradient 5.9e-08 / 2.1e-07;
tsrl_iqn_select's q is 0 ulp from the rounded f64 mean and no row is excluded.
"""


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "iqn.npz"))


def _dev_of(got, ref64):
    scale = float(ref64.abs().max()) or 1.0
    return float((got.double() - ref64).abs().max()) / scale


# -- embed -----------------------------------------------------------------------------------------
EMB_CASES = [(B, N, D, C) for B in (1, 3, 65) for N in (2, 8, 33) for D in (1, 64, 65, 200)
             for C in (1, 64, 65)] + [(2, 2, 3136, 64), (3, 9, 70, _C.IQN_MAX_COSINES)]
EMB_NAMES = ("e", "out", "g_h", "g_W", "g_b", "g_z")


def embed_inputs(B, N, D, C, dev):
    g = torch.Generator().manual_seed(1000003 * B + 10007 * N + 101 * D + C)
    h = torch.randn(B, D, generator=g)
    taus = torch.rand(B, N, generator=g)
    taus[0, 0] = 0.0
    taus[-1, -1] = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    k = 1.0 / np.sqrt(C)
    W = (torch.rand(D, C, generator=g) * 2 - 1) * k
    bias = (torch.rand(D, generator=g) * 2 - 1) * k
    g_out = torch.randn(B * N, D, generator=g)
    return tuple(t.to(dev).contiguous() for t in (h, taus, W, bias, g_out))


def embed_composition(h, taus, W, bias, g_out, dtype):
    """discrete.py:143-155, 211-212 and its autograd in ``dtype``, over the f32 cos argument:
    (e, out, g_h, g_W, g_b, g_z)."""
    (B, D), N, C = h.shape, taus.shape[1], W.shape[1]
    h_, W_, b_ = (t.detach().to(dtype).requires_grad_(True) for t in (h, W, bias))
    i_pi = np.pi * torch.arange(start=1, end=C + 1, dtype=taus.dtype, device=taus.device) \
        .view(1, 1, C)
    arg = taus.view(B, N, 1) * i_pi
    assert arg.dtype == torch.float32
    zz = torch.addmm(b_, torch.cos(arg.to(dtype)).view(B * N, C), W_.t())
    zz.retain_grad()
    e = torch.relu(zz)
    out = (h_.unsqueeze(1) * e.view(B, N, D)).view(B * N, D)
    out.backward(g_out.to(dtype))
    return e.detach(), out.detach(), h_.grad, W_.grad, b_.grad, zz.grad


def embed_kernels(h, taus, W, bias, g_out):
    """The two entry points as they stand (g_b from the backward's own f64 fold), the weight
    gradient through _linear_grads: (e, out, g_h, g_W, g_b, g_z, cosine features)."""
    (B, D), N, C = h.shape, taus.shape[1], W.shape[1]
    L, s = _C.lib(), _C.stream_ptr(h.device)
    e = torch.full((B * N, D), 7.0, device=h.device)
    out, g_z = torch.full_like(e, 7.0), torch.full_like(e, 7.0)
    g_h = torch.full_like(h, 7.0)
    cos = torch.full((B * N, C), 7.0, device=h.device)
    _C.check(L.tsrl_iqn_embed_fwd(_C.ptr(h), _C.ptr(taus), _C.ptr(W), _C.ptr(bias), B, N, D, C,
                                  _C.ptr(e), _C.ptr(out), s), "tsrl_iqn_embed_fwd")
    g_b = torch.full_like(bias, 7.0)
    part = torch.empty(B, D, dtype=torch.float64, device=h.device)
    _C.check(L.tsrl_iqn_embed_bwd(_C.ptr(g_out), _C.ptr(e), _C.ptr(h), _C.ptr(taus), B, N, D, C,
                                  _C.ptr(g_h), _C.ptr(g_z), _C.ptr(cos), _C.ptr(part),
                                  _C.ptr(g_b), s), "tsrl_iqn_embed_bwd")
    with torch.no_grad():
        _, g_W, _ = _linear_grads(cos, W, g_z, False, True, False)
    return e, out, g_h, g_W, g_b, g_z, cos


@pytest.mark.parametrize("B,N,D,C", EMB_CASES)
def test_embed_matches_f64(dev, B, N, D, C):
    """Measured on an MI355X (max over the 110 cases, deviation from f64 over max|ref|, kernel /
    torch f32): e 5.4e-08 / 7.0e-07, out 5.9e-08 / 4.6e-07, g_h 1.5e-07 / 8.0e-07, g_W 1.7e-06 /
    1.7e-06, g_b 5.8e-08 / 8.6e-07, g_z 5.6e-08 / 5.6e-08; largest ratio in one case 1.9 (g_W)."""
    args = embed_inputs(B, N, D, C, dev)
    h, taus, W, bias, g_out = args
    ref = embed_composition(*args, torch.float64)
    f32 = embed_composition(*args, torch.float32)
    *got, cos = embed_kernels(*args)
    figures = []
    for name, k, t, r in zip(EMB_NAMES, got, f32, ref):
        assert k.shape == r.shape and k.dtype == torch.float32, name
        figures.append((name, _dev_of(k, r), _dev_of(t, r)))
    print(f"embed B {B} N {N} D {D} C {C}: kernel / torch-f32 deviation from f64 over "
          "max|ref|: " + ", ".join(f"{n} {k:.2e} / {t:.2e}" for n, k, t in figures))
    for name, k, t in figures:
        assert k <= 4 * t, (name, k, t)
    # the cosine features are the f32 composition's within an ulp of a value in [-1, 1]
    assert float((cos.double() - torch.cos((taus.view(B, N, 1) * (np.pi * torch.arange(
        1, C + 1, dtype=torch.float32, device=dev))).double()).view(B * N, C)).abs().max()) \
        <= 2.0 ** -24
    # two runs, the same bits
    for a, b2 in zip(got, embed_kernels(*args)[:6]):
        assert torch.equal(a, b2)
    # the autograd Function is these two launches
    h_, W_, b_ = (t.clone().requires_grad_(True) for t in (h, W, bias))
    out = _IQNEmbedFn.apply(h_, taus, W_, b_)
    out.backward(g_out)
    assert torch.equal(out.detach(), got[1]) and torch.equal(h_.grad, got[2])
    assert torch.equal(W_.grad, got[3]) and torch.equal(b_.grad, got[4])

    # z == 0 everywhere: e, out and g_z exactly 0 (torch's ReLU backward is zero at 0)
    zero = embed_kernels(h, taus, torch.zeros_like(W), torch.zeros_like(bias), g_out)
    for name, t in zip(EMB_NAMES, zero[:6]):
        assert (t == 0).all(), name

    # one NaN in h poisons that row's outputs at that feature and nothing else
    r, d = B // 2, D // 2
    h_nan = h.clone()
    h_nan[r, d] = float("nan")
    bad = embed_kernels(h_nan, taus, W, bias, g_out)
    rows = torch.arange(r * N, (r + 1) * N, device=dev)
    hit = torch.zeros(B * N, D, dtype=torch.bool, device=dev)
    hit[rows, d] = True
    assert torch.equal(bad[0], got[0])                       # e does not read h
    assert bad[1][hit].isnan().all() and torch.equal(bad[1][~hit], got[1][~hit])
    assert torch.equal(bad[2], got[2])                       # g_h = sum g_out e
    live = hit & (got[0] > 0)
    assert bad[5][live].isnan().all() and torch.equal(bad[5][~live], got[5][~live])
    assert torch.isfinite(bad[3][torch.arange(D, device=dev) != d]).all()


def test_embed_argument_errors_and_empty_batch(dev):
    h, taus, W, bias, g_out = embed_inputs(2, 3, 5, 4, dev)
    L, s = _C.lib(), _C.stream_ptr(dev)
    e = torch.full((6, 5), 7.0, device=dev)
    out = torch.full_like(e, 7.0)
    wide = torch.zeros(5, _C.IQN_MAX_COSINES + 1, device=dev)
    rc = L.tsrl_iqn_embed_fwd(_C.ptr(h), _C.ptr(taus), _C.ptr(wide), _C.ptr(bias), 2, 3, 5,
                              _C.IQN_MAX_COSINES + 1, _C.ptr(e), _C.ptr(out), s)
    assert rc != 0
    assert (e == 7.0).all() and (out == 7.0).all()           # nothing was launched
    assert L.tsrl_iqn_embed_fwd(None, None, None, None, 0, 3, 5, 4, None, None, s) == 0
    assert L.tsrl_iqn_embed_bwd(None, None, None, None, 0, 3, 5, 4, None, None, None, None,
                                None, s) == 0
    g_z, g_h = torch.empty_like(e), torch.empty_like(h)
    assert L.tsrl_iqn_embed_bwd(_C.ptr(g_out), _C.ptr(e), _C.ptr(h), None, 2, 3, 5, 4,
                                _C.ptr(g_h), _C.ptr(g_z), None, None, _C.ptr(bias), s) != 0
    assert L.tsrl_iqn_embed_fwd(_C.ptr(h), None, _C.ptr(W), _C.ptr(bias), 2, 3, 5, 4, _C.ptr(e),
                                _C.ptr(out), s) != 0


def test_module_takes_the_kernel_up_to_the_cosine_limit(dev):
    """C == IQN_MAX_COSINES runs the fused Function, C + 1 the torch composition; both agree
    with the module's own torch lines."""
    torch.manual_seed(0)
    for C, fused in ((_C.IQN_MAX_COSINES, True), (_C.IQN_MAX_COSINES + 1, False)):
        emb = CosineEmbeddingNetwork(C, 24).to(dev)
        h = torch.randn(5, 24, device=dev, requires_grad=True)
        taus = torch.rand(5, 6, device=dev)
        out = emb.hadamard(h, taus)
        assert (type(out.grad_fn).__name__ == "_IQNEmbedFnBackward") == fused
        want = (h.unsqueeze(1) * emb(taus)).view(30, 24)
        torch.testing.assert_close(out, want, rtol=1e-5, atol=1e-6)
        g = torch.randn(30, 24, device=dev)
        got = torch.autograd.grad(out, (h, emb.net[0].weight, emb.net[0].bias), g)
        ref = torch.autograd.grad(want, (h, emb.net[0].weight, emb.net[0].bias), g)
        for a, b2 in zip(got, ref):
            torch.testing.assert_close(a, b2, rtol=1e-4, atol=1e-5)
    # fused = False and a create_graph pass keep to differentiable torch ops
    emb = CosineEmbeddingNetwork(8, 24).to(dev)
    h = torch.randn(5, 24, device=dev, requires_grad=True)
    taus = torch.rand(5, 6, device=dev)
    assert type(emb.hadamard(h, taus, fused=False).grad_fn).__name__ != "_IQNEmbedFnBackward"
    out = emb.hadamard(h, taus)
    (g_h,) = torch.autograd.grad(out.sum(), h, create_graph=True)
    assert g_h.requires_grad
    want = torch.autograd.grad((h.unsqueeze(1) * emb(taus)).sum(), h)[0]
    torch.testing.assert_close(g_h, want, rtol=1e-5, atol=1e-6)
    g_h.sum().backward()
    assert emb.net[0].weight.grad is not None


# -- select ----------------------------------------------------------------------------------------
SEL_BS = (1, 63, 65)
SEL_AS = (1, 2, 18)
SEL_NM = ((2, 2), (8, 8), (5, 7), (65, 3), (32, 200))


def select_inputs(b, A, N, M):
    """CPU tensors (sel [b, A, N], eval [b, A, M]) of one case."""
    g = torch.Generator().manual_seed(100000 * b + 1000 * A + 10 * N + M)
    return torch.randn(b, A, N, generator=g), torch.randn(b, A, M, generator=g)


def top2_rel_gap(q64):
    """Per row (best - second) / max(|best|, |second|) of an f64 [b, A] table; inf at A 1."""
    if q64.shape[1] < 2:
        return torch.full((q64.shape[0],), float("inf"), dtype=torch.float64)
    top = q64.topk(2, dim=1)[0]
    return (top[:, 0] - top[:, 1]) / top.abs().max(dim=1)[0]


def _ulp(x32):
    ax = x32.abs()
    return torch.nextafter(ax, torch.full_like(ax, float("inf"))) - ax


def layout(t, major, dev):
    """``t`` [b, A, N] on the device, contiguous ("action") or as the transposed view of a
    contiguous [b, N, A] ("quantile"), which is what the network's head returns."""
    t = t.to(dev)
    if major == "action":
        return t.contiguous()
    v = t.transpose(1, 2).contiguous().transpose(1, 2)
    assert v.shape == t.shape and (not v.is_contiguous() or 1 in v.shape[1:])
    return v


@pytest.mark.parametrize("major", ("action", "quantile"))
@pytest.mark.parametrize("N,M", SEL_NM)
@pytest.mark.parametrize("A", SEL_AS)
@pytest.mark.parametrize("b", SEL_BS)
def test_select_matches_f64(dev, b, A, N, M, major):
    sel, ev = select_inputs(b, A, N, M)
    q64 = sel.double().mean(2)
    keep = (top2_rel_gap(q64) >= 1e-6).to(dev)
    assert int((~keep).sum()) <= b // 100
    act_ref = torch.as_tensor(q64.numpy().argmax(axis=1), device=dev)
    sel, ev = layout(sel, major, dev), layout(ev, major, dev)
    q, act, row = iqn_select(sel, ev, want_q=True, want_row=True)
    ref32 = q64.float().to(dev)
    worst = ((q - ref32).abs() / _ulp(ref32)).max().item()
    print(f"select b {b} A {A} N {N} M {M} {major}: q max {worst:.2f} ulp, rows kept "
          f"{int(keep.sum())}/{b}")
    assert worst <= 2.0
    assert act.dtype == torch.int64 and torch.equal(act[keep], act_ref[keep])
    rows = torch.arange(b, device=dev)
    assert row.shape == (b, M) and torch.equal(row, ev[rows, act])
    # eval null: sel's own row; outputs not asked for are not written
    q2, act2, row2 = iqn_select(sel, None, want_row=True)
    assert q2 is None and torch.equal(act2, act)
    assert row2.shape == (b, N) and torch.equal(row2, sel[rows, act])
    q3, act3, row3 = iqn_select(sel, ev, want_q=True, want_act=False)
    assert act3 is None and row3 is None and torch.equal(q3, q)
    # the two layouts of sel and eval may differ
    other = "quantile" if major == "action" else "action"
    q4, act4, row4 = iqn_select(sel, layout(ev.cpu(), other, dev), want_q=True, want_row=True)
    assert torch.equal(q4, q) and torch.equal(act4, act) and torch.equal(row4, row)


@pytest.mark.parametrize("major", ("action", "quantile"))
def test_select_constructed_rows(dev, major):
    b, A, N, M = 70, 6, 65, 9
    g = torch.Generator().manual_seed(5)
    sel = torch.randn(b, A, N, generator=g)
    sel[0:10, 4] = sel[0:10, 2] = sel[0:10, 1] + 1.0     # ties among the maxima: 2 before 4
    sel[0:10, 1] -= 3.0
    sel[10:20] = 0.25                                     # constant rows: action 0
    sel[20:30, 3, 7] = float("nan")                       # one NaN action beats every number
    sel[30:40, 5, 0] = sel[30:40, 2, 64] = float("nan")   # the first NaN wins
    sel[40:50, 0] = 50.0                                  # the maximum at the first action
    sel[50:60, 5] = 50.0                                  # and at the last (another wave's)
    ev = torch.randn(b, A, M, generator=g)
    sel, ev = layout(sel, major, dev), layout(ev, major, dev)
    rows = torch.arange(b, device=dev)
    q, act, row = iqn_select(sel, ev, want_q=True, want_row=True)
    assert act[0:10].tolist() == [2] * 10 and torch.equal(q[0:10, 2], q[0:10, 4])
    assert act[10:20].tolist() == [0] * 10
    assert act[20:30].tolist() == [3] * 10 and bool(q[20:30, 3].isnan().all())
    assert act[30:40].tolist() == [2] * 10
    assert act[40:50].tolist() == [0] * 10 and act[50:60].tolist() == [5] * 10
    assert torch.equal(row, ev[rows, act])
    # the argmax is torch's on the rounded means
    assert torch.equal(act, q.max(dim=1)[1])
    one = torch.full((3, 1, N), float("-inf"), device=dev)
    assert iqn_select(one)[1].tolist() == [0, 0, 0]
    q, act, row = iqn_select(sel[:0], None, want_q=True, want_row=True)
    assert q.shape == (0, A) and act.shape == (0,) and row.shape == (0, N)


def test_select_refuses_other_strides(dev):
    sel = torch.randn(4, 3, 8, device=dev)
    L = _C.lib()
    act = torch.full((4,), -5, dtype=torch.int64, device=dev)
    rc = L.tsrl_iqn_select(_C.ptr(sel), 16, 2, None, 0, 0, 4, 3, 4, 4, None, _C.ptr(act), None,
                           _C.stream_ptr(dev))
    assert rc != 0 and (act == -5).all()
    # a view that is neither layout is copied by the binding
    wide = torch.randn(4, 3, 16, device=dev)[:, :, ::2]
    assert torch.equal(iqn_select(wide)[1], wide.mean(2).argmax(1))


# -- loss ------------------------------------------------------------------------------------------
LOSS_BS = (1, 63, 64, 65, 257)
LOSS_AS = (1, 6)
LOSS_NM = ((2, 2), (8, 8), (5, 7), (7, 5), (64, 65), (300, 3), (3, 300))


def iqn_reference(curr, act, returns, taus, weight):
    """iqn.py:93-108 in the dtype of ``curr``; returns (loss, prio, d loss / d curr)."""
    curr = curr.detach().clone().requires_grad_(True)
    b, _, N = curr.shape
    M = returns.shape[1]
    ca = curr[torch.arange(b, device=curr.device), act, :].unsqueeze(2)
    target = returns.unsqueeze(1)
    diff = F.smooth_l1_loss(target.expand(-1, N, -1), ca.expand(-1, -1, M), reduction="none")
    huber = (diff * (taus.unsqueeze(2) - (target - ca).detach().le(0.).to(curr.dtype)).abs()) \
        .sum(-1).mean(1)
    loss = (huber * (1.0 if weight is None else weight)).mean()
    prio = diff.detach().abs().sum(-1).mean(1)
    loss.backward()
    return loss.detach(), prio, curr.grad


def _f64(*ts):
    return tuple(None if t is None else (t.double() if t.is_floating_point() else t)
                 for t in ts)


def loss_inputs(b, A, N, M, dev, weighted):
    g = torch.Generator().manual_seed(17 * b + 5 * A + 1000 * N + M + int(weighted))
    curr = torch.randn(b, A, N, generator=g)
    act = torch.randint(0, A, (b,), generator=g)
    returns = 2.0 * torch.randn(b, M, generator=g)  # |u| below and above the Huber knee
    taus = torch.rand(b, N, generator=g)
    weight = torch.rand(b, generator=g) + 0.1 if weighted else None
    d = lambda t: None if t is None else t.to(dev).contiguous()  # noqa: E731
    return curr, d(act), d(returns), d(taus), d(weight)


def _iqn_kernel(curr, act, returns, taus, weight):
    x = curr.detach().requires_grad_(True)  # a leaf with the strides of ``curr``
    loss, prio = _IQNLoss.apply(x, (act, returns, taus, weight, None, None))
    loss.backward()
    assert x.grad.shape == curr.shape
    return loss.detach().clone(), prio.clone(), x.grad.clone()


def _assert_loss_outputs(got, ref64, what):
    """loss rtol 1e-5, per-row vector rtol 1e-5, gradient rtol 1e-4; atol 1e-6 max|ref|."""
    for (g, r, rtol, name) in zip(got, ref64, (1e-5, 1e-5, 1e-4), ("loss", "prio", "grad")):
        atol = 1e-6 * float(r.abs().max())
        torch.testing.assert_close(g.double(), r, rtol=rtol, atol=atol, msg=lambda m: f"{what} "
                                   f"{name}: {m}")


@pytest.mark.parametrize("N,M", LOSS_NM)
@pytest.mark.parametrize("A", LOSS_AS)
@pytest.mark.parametrize("b", LOSS_BS)
def test_loss_matches_f64(dev, b, A, N, M):
    for weighted in (False, True):
        curr_cpu, act, returns, taus, weight = loss_inputs(b, A, N, M, dev, weighted)
        results = []
        for major in ("action", "quantile"):
            curr = layout(curr_cpu, major, dev)
            args = (curr, act, returns, taus, weight)
            ref = iqn_reference(*_f64(*args))
            got = _iqn_kernel(*args)
            if major == "action":
                f32 = iqn_reference(*args)
                print(f"loss b {b} A {A} N {N} M {M} w {int(weighted)}: kernel / torch-f32 "
                      "deviation from f64, over max|ref|: " + ", ".join(
                          f"{n} {_dev_of(k, r):.2e} / {_dev_of(t, r):.2e}"
                          for n, k, t, r in zip(("loss", "prio", "grad"), got, f32, ref)))
            _assert_loss_outputs(got, ref, f"iqn b {b} A {A} N {N} M {M} {major}")
            grad = got[2]
            off = torch.ones_like(grad, dtype=torch.bool)
            off[torch.arange(b, device=dev), act] = False
            assert (grad[off] == 0).all()
            for a, c in zip(got, _iqn_kernel(*args)):  # two runs, the same bits
                assert torch.equal(a, c)
            results.append(got)
        for a, c in zip(*results):  # the layout changes no value
            assert torch.equal(a, c)


def test_loss_gradient_keeps_the_layout_it_was_given(dev):
    curr_cpu, act, returns, taus, weight = loss_inputs(9, 6, 8, 8, dev, True)
    head = curr_cpu.transpose(1, 2).contiguous().to(dev).requires_grad_(True)   # [b, N, A]
    loss, _ = _IQNLoss.apply(head.transpose(1, 2), (act, returns, taus, weight, None, None))
    saved = loss.grad_fn.saved_tensors[0]
    assert saved.shape == (9, 6, 8) and saved.stride() == (48, 1, 6)  # no transposing copy
    loss.backward()
    ref = iqn_reference(head.detach().transpose(1, 2).double(), act, returns.double(),
                        taus.double(), weight.double())
    assert head.grad.shape == (9, 8, 6) and head.grad.is_contiguous()
    torch.testing.assert_close(head.grad.double(), ref[2].transpose(1, 2), rtol=1e-4,
                               atol=1e-6 * float(ref[2].abs().max()))


@pytest.mark.parametrize("major", ("action", "quantile"))
def test_loss_constructed_rows(dev, major):
    # N = 2, M = 3; every u is exact in f32
    curr = torch.tensor([[[0.0, 0.5], [9.0, 9.0]],       # tau = 0 and u = 0 exactly
                         [[9.0, 9.0], [0.0, 0.0]],       # |u| >> 1
                         [[1.0, -1.0], [9.0, 9.0]],      # |u| == 1 on both sides
                         [[0.0, 0.0], [0.0, 0.0]]])      # an out-of-range action
    act = torch.tensor([0, 1, 0, 2], device=dev)
    returns = torch.tensor([[0.0, 1.0, 0.5], [100.0, -100.0, 100.0], [0.0, 0.0, 0.0],
                            [1.0, 2.0, 3.0]], device=dev)
    taus = torch.tensor([[0.0, 0.75], [0.25, 0.5], [0.25, 0.75], [0.5, 0.5]], device=dev)
    b, N = 4, 2
    loss, prio, grad = _iqn_kernel(layout(curr, major, dev), act, returns, taus, None)
    f32 = lambda *xs: [float(np.float32(x)) for x in xs]  # noqa: E731
    # row 0, i = 0 (theta 0, tau 0): u = (0, 1, 1/2): h = (0, 1/2, 1/8); u == 0 counts as
    # <= 0, so k = (1, 0, 0): nothing is left of the loss and of the gradient (the u == 0 pair
    # has derivative 0).  i = 1 (theta 1/2, tau 3/4): u = (-1/2, 1/2, 0), k = (1/4, 3/4, 1/4)
    assert prio[0].item() == (0.5 + 0.125 + 0.125 + 0.125) / N
    assert grad[0, 0].tolist() == f32(0.0, -(-0.5 * 0.25 + 0.5 * 0.75) / (b * N))
    # row 1: h = |u| - 1/2 = 99.5, the derivative clamped to +-1
    assert prio[1].item() == 6 * 99.5 / N
    assert grad[1, 1].tolist() == f32(-(0.25 - 0.75 + 0.25) / (b * N),
                                      -(0.5 - 0.5 + 0.5) / (b * N))
    # row 2: |u| == 1 sits on the quadratic and the linear branch alike
    assert prio[2].item() == 6 * 0.5 / N
    assert grad[2, 0].tolist() == f32(-(-3 * 0.75) / (b * N), -(3 * 0.75) / (b * N))
    # row 3: NaN priority and loss, its whole gradient block zero, the other rows untouched
    assert bool(prio[3].isnan()) and bool(loss.isnan()) and (grad[3] == 0).all()
    assert (grad[0, 1] == 0).all() and (grad[1, 0] == 0).all() and (grad[2, 1] == 0).all()
    ok = torch.tensor([0, 1, 2], device=dev)
    ref = iqn_reference(*_f64(curr.to(dev)[ok], act[ok], returns[ok], taus[ok], None))
    got = _iqn_kernel(layout(curr[:3], major, dev), act[ok], returns[ok], taus[ok], None)
    _assert_loss_outputs(got, ref, "constructed")
    for bad in (-1, 2):
        act_bad = act.clone()
        act_bad[1] = bad
        loss_b, prio_b, grad_b = _iqn_kernel(layout(curr, major, dev), act_bad, returns, taus,
                                             None)
        assert bool(prio_b[1].isnan()) and (grad_b[1] == 0).all()
        assert torch.equal(grad_b[[0, 2]], grad[[0, 2]]) and torch.equal(prio_b[0], prio[0])


@pytest.mark.parametrize("major", ("action", "quantile"))
def test_loss_non_finite_targets_follow_torch(dev, major):
    curr_cpu, act, returns, taus, weight = loss_inputs(8, 6, 5, 7, dev, True)
    returns = returns.clone()
    returns[2, 3] = float("nan")
    returns[5, 0] = float("inf")
    curr = layout(curr_cpu, major, dev)
    loss, prio, grad = _iqn_kernel(curr, act, returns, taus, weight)
    ref = iqn_reference(*_f64(curr, act, returns, taus, weight))
    assert bool(loss.isnan()) and bool(ref[0].isnan())
    assert torch.equal(prio.isnan(), ref[1].isnan()) and prio.isnan().tolist() == \
        [False, False, True, False, False, False, False, False]
    assert bool(prio[5].isinf()) and bool(ref[1][5].isinf())
    # the NaN target keeps its NaN in the derivative of every quantile of its row; the
    # infinite one is clamped to 1
    assert torch.equal(grad.isnan(), ref[2].isnan())
    assert grad[2, act[2]].isnan().all() and torch.isfinite(grad[5]).all()
    fin = ~ref[2].isnan()
    torch.testing.assert_close(grad[fin].double(), ref[2][fin], rtol=1e-4,
                               atol=1e-6 * float(ref[2][fin].abs().max()))
    fin = ~ref[1].isnan() & ~ref[1].isinf()
    torch.testing.assert_close(prio[fin].double(), ref[1][fin], rtol=1e-5, atol=0)


def test_loss_argument_errors_launch_nothing(dev):
    L, s = _C.lib(), _C.stream_ptr(dev)
    b, A = 2, 3
    for N, M in ((1, 4), (4, 1), (_C.DIST_MAX_N + 1, 4), (4, _C.DIST_MAX_N + 1)):
        curr = torch.zeros(b, A, N, device=dev)
        act = torch.zeros(b, dtype=torch.int64, device=dev)
        returns, taus = torch.zeros(b, M, device=dev), torch.zeros(b, N, device=dev)
        grad = torch.full_like(curr, 7.0)
        prio = torch.full((b,), 7.0, device=dev)
        loss = torch.full((), 7.0, device=dev)
        parts = torch.full((b,), 7.0, dtype=torch.float64, device=dev)
        rc = L.tsrl_iqn_loss_fwd_bwd(_C.ptr(curr), N, 1, _C.ptr(act), _C.ptr(returns),
                                     _C.ptr(taus), None, b, A, N, M, _C.ptr(grad), _C.ptr(prio),
                                     _C.ptr(parts), _C.ptr(loss), s)
        assert rc != 0, (N, M)
        assert (grad == 7.0).all() and (prio == 7.0).all() and loss.item() == 7.0
        with pytest.raises(_C.TsrlError):
            _IQNLoss.apply(curr, (act, returns, taus, None, None, None))
    # b == 1 needs no partials
    curr_cpu, act, returns, taus, _ = loss_inputs(1, 6, 8, 8, dev, False)
    got = _iqn_kernel(curr_cpu.to(dev), act, returns, taus, None)
    _assert_loss_outputs(got, iqn_reference(*_f64(curr_cpu.to(dev), act, returns, taus, None)),
                         "b 1")


@pytest.mark.parametrize("b,A,N", ((1, 1, 2), (65, 6, 8), (257, 6, 200), (63, 2, 300)))
def test_loss_equals_qr_loss_at_fixed_fractions(dev, b, A, N):
    """M == N and every row's fractions tau_hat: tsrl_qr_loss_fwd_bwd's outputs bit for bit."""
    for weighted in (False, True):
        curr_cpu, act, returns, _, weight = loss_inputs(b, A, N, N, dev, weighted)
        tau = torch.linspace(0, 1, N + 1)
        tau_hat = ((tau[:-1] + tau[1:]) / 2).to(dev).contiguous()
        x = curr_cpu.to(dev).requires_grad_(True)
        loss, prio = _QRLoss.apply(x, (act, returns, tau_hat, weight, None, None))
        loss.backward()
        taus = tau_hat.repeat(b, 1).contiguous()
        for major in ("action", "quantile"):
            got = _iqn_kernel(layout(curr_cpu, major, dev), act, returns, taus, weight)
            assert torch.equal(got[0], loss.detach()) and torch.equal(got[1], prio)
            assert torch.equal(got[2], x.grad)


def test_loss_seed_paths_and_static_outputs(dev):
    from tianshou_amd.policy.onpolicy import _unit_seed
    curr_cpu, act, returns, taus, weight = loss_inputs(257, 6, 5, 7, dev, True)
    curr = layout(curr_cpu, "quantile", dev)
    args = (act, returns, taus, weight, None, None)
    grads = []
    for seed in ("ones", "unit", 2.5):
        x = curr.detach().requires_grad_(True)
        loss, vec = _IQNLoss.apply(x, args)
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
    vec_out = torch.empty(257, device=dev)
    loss_out = torch.empty((), device=dev)
    loss, vec = _IQNLoss.apply(curr.detach().requires_grad_(True),
                               args[:-2] + (vec_out, loss_out))
    assert vec.data_ptr() == vec_out.data_ptr() and torch.equal(loss.detach(), loss_out)
    assert torch.equal(vec_out, _IQNLoss.apply(curr, args)[1])


# -- update() against the recording ----------------------------------------------------------------
from tests import test_gpu_dqn as gd  # noqa: E402  (its buffer / recorder helpers)

TAGS = ("target", "uneven", "notarget", "per", "rms")
ADAM_TAGS = ("target", "uneven", "notarget", "per")


def _cfg(z):
    return json.loads(str(z["learn_cfg"]))


def _init_state(z):
    return {k[len("init_"):]: torch.as_tensor(z[k]) for k in z.files if k.startswith("init_")}


def _policy(z, cfg, tag, dev, optim=None, **attrs):
    v, n = cfg["variants"][tag], cfg["net"]
    feature = Net(cfg["D"], n["feature_out"], hidden_sizes=n["feature_hidden"], device=dev)
    net = ImplicitQuantileNetwork(feature, cfg["A"], hidden_sizes=n["head_hidden"],
                                  num_cosines=n["num_cosines"], device=dev).to(dev)
    net.load_state_dict(_init_state(z), strict=True)
    opt = {"rms": lambda p: torch.optim.RMSprop(p, lr=7e-4, eps=1e-5, alpha=0.99),
           "adam": lambda p: torch.optim.Adam(p, lr=1e-3),
           "sgd": lambda p: torch.optim.SGD(p, lr=1e-2)}[optim or v["optim"]](net.parameters())
    policy = IQNPolicy(net, opt, discount_factor=cfg["gamma"], sample_size=cfg["sample_size"],
                       online_sample_size=v["N"], target_sample_size=v["M"],
                       estimation_step=v["n_step"], target_update_freq=v["freq"]).to(dev)
    for k, a in attrs.items():
        setattr(policy, k, a)
    policy.train()
    return policy, v


def _inject(policy, z, tag, dev, step):
    """The recorded draws of update ``step[0]`` through ``_sample_taus``, in their order."""
    def taus(shape, device):
        d = torch.as_tensor(z[f"{tag}_u{step[0]}_draw{step[1]}"]).to(device)
        assert tuple(shape) == tuple(d.shape), (tag, step, shape)
        step[1] += 1
        return d
    policy._sample_taus = taus


def _run_variant(z, dev, tag, check_params, **attrs):
    cfg = _cfg(z)
    policy, v = _policy(z, cfg, tag, dev, **attrs)
    buf = gd._filled_buffer(z, cfg, dev, per=bool(v.get("per")))
    seen = gd._record(policy)
    step = [0, 0]
    _inject(policy, z, tag, dev, step)
    np.random.seed(cfg["seed"])
    for u in range(cfg["updates"]):
        step[:] = [u, 0]
        res = policy.update(v["bs"], buf)
        assert step[1] == (3 if v["freq"] else 2)
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
    assert policy._iter == cfg["updates"]
    return policy


def _adam_check(z, tag):
    def check(u, policy):
        for k, t in policy.model.state_dict().items():
            np.testing.assert_allclose(t.cpu().numpy(), z[f"{tag}_u{u}_param_{k}"], rtol=1e-5,
                                       atol=1e-6, err_msg=f"{tag} update {u} {k}")
    return check


@pytest.mark.parametrize("leg", ("graph", "eager", "torch"))
@pytest.mark.parametrize("tag", ADAM_TAGS)
def test_update_matches_reference_adam(z, dev, tag, leg):
    attrs = {"graph": dict(fused=True, graph_learn=True),
             "eager": dict(fused=True, graph_learn=False), "torch": dict(fused=False)}[leg]
    policy = _run_variant(z, dev, tag, _adam_check(z, tag), **attrs)
    nets = [policy.model] + ([policy.model_old] if policy._target else [])
    assert all(n.fused_embed == (leg != "torch") for n in nets)
    if leg == "torch":
        assert policy._flat is None and not policy._learn_graphs
        return
    assert policy._flat is not None and policy._flat.adam_bound(policy.optim)
    assert not policy._graph_failed
    # captured once (the second update is the first to replay) and reused: only the draws change
    assert len(policy._learn_graphs) == (1 if leg == "graph" else 0)


def test_update_matches_reference_rmsprop(z, dev):
    """The fused legs' max |parameter - recorded| after each update stays within 4 x the torch
    formulation's on the same GPU (all printed)."""
    torch_dev = []
    _run_variant(z, dev, "rms", lambda u, p: torch_dev.append(
        gd._param_dev(p.model, z, f"rms_u{u}_param_")), fused=False)
    for leg, graph in (("graph", True), ("eager", False)):
        fused_dev = []
        policy = _run_variant(z, dev, "rms", lambda u, p: fused_dev.append(
            gd._param_dev(p.model, z, f"rms_u{u}_param_")), fused=True, graph_learn=graph)
        print("rms max|dparam| per update: torch", torch_dev, leg, fused_dev)
        assert policy._flat.adam_bound(policy.optim)
        assert bool(policy._learn_graphs) == graph
        for u in range(len(torch_dev)):
            assert fused_dev[u] <= 4 * torch_dev[u], (leg, u, fused_dev[u], torch_dev[u])


def _updates(z, dev, tag, **attrs):
    cfg = _cfg(z)
    policy, v = _policy(z, cfg, tag, dev, fused=True, **attrs)
    buf = gd._filled_buffer(z, cfg, dev, per=bool(v.get("per")))
    step = [0, 0]
    _inject(policy, z, tag, dev, step)
    np.random.seed(cfg["seed"])
    out = []
    for u in range(cfg["updates"]):
        step[:] = [u, 0]
        loss = policy.update(v["bs"], buf)["loss"]
        out.append((loss, [p.detach().clone() for p in policy.model.parameters()]))
    return policy, out


@pytest.mark.parametrize("tag", TAGS)
def test_graph_replay_is_bitwise_eager(z, dev, tag):
    pol_g, out_g = _updates(z, dev, tag, graph_learn=True)
    pol_e, out_e = _updates(z, dev, tag, graph_learn=False)
    assert len(pol_g._learn_graphs) == 1 and not pol_e._learn_graphs
    for (loss_g, par_g), (loss_e, par_e) in zip(out_g, out_e):
        assert loss_g == loss_e
        for a, b2 in zip(par_g, par_e):
            assert torch.equal(a, b2)


def test_learn_graph_is_captured_once(z, dev, monkeypatch):
    from tianshou_amd.policy import dqn as dqn_mod
    captures = []
    capture = dqn_mod.graph_capture

    def counting(graph):
        captures.append(graph)
        return capture(graph)

    monkeypatch.setattr(dqn_mod, "graph_capture", counting)
    policy, out = _updates(z, dev, "target", graph_learn=True)
    assert len(captures) == 1 and len(policy._learn_graphs) == 1
    assert len({loss for loss, _ in out}) == len(out)  # the replays saw fresh draws and rows


# -- other paths -----------------------------------------------------------------------------------
def test_reference_checkpoint_loads_strict_and_gives_the_recorded_loss(z, dev, tmp_path):
    cfg = _cfg(z)
    path = os.path.join(tmp_path, "iqn_reference.pth")
    torch.save(_init_state(z), path)
    v, n = cfg["variants"]["target"], cfg["net"]
    torch.manual_seed(99)  # other initial weights than the checkpoint's
    feature = Net(cfg["D"], n["feature_out"], hidden_sizes=n["feature_hidden"], device=dev)
    net = ImplicitQuantileNetwork(feature, cfg["A"], hidden_sizes=n["head_hidden"],
                                  num_cosines=n["num_cosines"], device=dev).to(dev)
    assert list(net.state_dict()) == json.loads(str(z["state_keys"]))
    res = net.load_state_dict(torch.load(path, map_location=dev), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    policy = IQNPolicy(net, torch.optim.Adam(net.parameters(), lr=1e-3),
                       discount_factor=cfg["gamma"], sample_size=cfg["sample_size"],
                       online_sample_size=v["N"], target_sample_size=v["M"],
                       estimation_step=v["n_step"], target_update_freq=v["freq"]).to(dev)
    policy.train()
    step = [0, 0]
    _inject(policy, z, "target", dev, step)
    buf = gd._filled_buffer(z, cfg, dev)
    np.random.seed(cfg["seed"])
    loss = policy.update(v["bs"], buf)["loss"]
    np.testing.assert_allclose(loss, float(z["target_u0_loss"]), rtol=2e-5)


def test_collector_runs_the_eager_device_step(dev):
    from tianshou_amd.data import Collector, VectorReplayBuffer
    from tianshou_amd.env import SyntheticVectorEnv
    E, T, D, A = 8, 16, 12, 6
    torch.manual_seed(0)
    np.random.seed(0)
    env = SyntheticVectorEnv(E, (D,), A, ep_len=10, device=dev, discrete=True)
    space = env.action_space
    feature = Net(D, 16, hidden_sizes=(16,), device=dev)
    net = ImplicitQuantileNetwork(feature, A, hidden_sizes=(16,), num_cosines=16,
                                  device=dev).to(dev)
    policy = IQNPolicy(net, torch.optim.Adam(net.parameters(), lr=1e-3), sample_size=12,
                       online_sample_size=5, target_sample_size=7, target_update_freq=4,
                       action_space=space).to(dev)
    sizes, sample = [], policy._sample_taus

    def rec(shape, device):
        sizes.append(tuple(shape))
        return sample(shape, device)

    policy._sample_taus = rec
    policy.eval()
    buf = VectorReplayBuffer(E * T * 2, E, device=dev)
    col = Collector(policy, env, buf)
    res = col.collect(n_step=E * T)
    assert res["n/st"] == E * T and len(buf) == E * T
    # every step drew its fractions: none was replayed from a graph; eval mode: sample_size
    assert sizes == [(E, 12)] * T
    policy.train()
    del sizes[:]
    np.random.seed(1)
    losses = [policy.update(32, buf)["loss"] for _ in range(3)]
    assert all(np.isfinite(losses)) and len(set(losses)) == 3
    assert sizes == [(32, 5), (32, 7), (32, 5)] * 3


def _graph_nodes(t):
    """The names of the autograd nodes behind ``t``."""
    seen, todo = set(), [t.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        todo.extend(f for f, _ in fn.next_functions)
    return {type(fn).__name__ for fn in seen}


def test_fused_false_reaches_the_embedding(z, dev):
    """``policy.fused = False`` is the reference's op sequence throughout: both networks'
    cosine embedding leaves the kernels too, and comes back with ``fused = True``."""
    from tianshou_amd.data import Batch
    policy, _ = _policy(z, _cfg(z), "target", dev)
    batch = Batch(obs=torch.as_tensor(z["add_obs"][:9]).to(dev), info=Batch())
    assert policy.fused and policy.model.fused_embed and policy.model_old.fused_embed
    assert "_IQNEmbedFnBackward" in _graph_nodes(policy(batch).logits)
    policy.fused = False
    assert not policy.model.fused_embed and not policy.model_old.fused_embed
    for model in ("model", "model_old"):
        for p in getattr(policy, model).parameters():
            p.requires_grad_(True)
        nodes = _graph_nodes(policy(batch, model=model).logits)
        # the embedding's nn.Linear is the networks' only plain addmm
        assert "_IQNEmbedFnBackward" not in nodes and "AddmmBackward0" in nodes
    policy.fused = True
    assert policy.model.fused_embed and policy.model_old.fused_embed
    assert "_IQNEmbedFnBackward" in _graph_nodes(policy(batch).logits)


def test_forward_sample_sizes_follow_the_mode(z, dev):
    from tianshou_amd.data import Batch
    policy, v = _policy(z, _cfg(z), "uneven", dev)
    obs = torch.as_tensor(z["add_obs"][:9]).to(dev)
    batch = Batch(obs=obs, obs_next=obs, info=Batch())
    policy.eval()
    res = policy(batch)
    assert res.logits.shape == (9, 6, 16) and res.taus.shape == (9, 16)
    assert res.act.dtype == torch.int64 and res.act.is_cuda
    assert torch.equal(res.act, res.logits.mean(2).argmax(1)) or \
        (top2_rel_gap(res.logits.double().mean(2).cpu()) < 1e-6).any()
    assert policy(batch, model="model_old", input="obs_next").taus.shape == (9, 7)
    policy.train()
    assert policy(batch).taus.shape == (9, 5)
    assert not policy.model_old.training
    # the head's output is handed on as the view it is
    assert res.logits.transpose(1, 2).is_contiguous()
