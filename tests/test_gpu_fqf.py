"""FQFPolicy / FractionProposalNetwork / FullQuantileFunction on the device path
(tianshou_amd/policy/fqf.py, utils/net.py, the tsrl_fqf_* kernels of csrc/dqn_dist.hip).

Kernels: against the f64 restatements of tests/test_fqf_host.py on the same f32 inputs, with the
torch f32 composition beside the kernel.  The project's bound: a kernel output may deviate from
f64 by at most 4 x what torch's f32 leg deviates, both as a fraction of max|ref|; the observed
figures (and the taus' distance from the rounded f64 result in ulp) are printed.  What is exact
is asserted exactly: taus[:, 0] == 0, taus non-decreasing, tau_hats bitwise torch's midpoint of
the kernel's taus, tsrl_fqf_select's row a copy, gradient_of_taus bitwise torch's f32 on a dyadic
grid where every comparison is exact (and ties of both kinds occur).

update() against tests/golden/fqf.npz (tools/gen_goldens.py gen_fqf; tests/test_fqf_host.py pins
that file) on the graph, eager and torch legs.  First the leg's own sa_quantile_hats /
sa_quantiles must lie within half the recorded min_margin of the recording, so every sign test
falls as the reference's did.  Then: indices equal, returns rtol 1e-5 / atol 1e-6, the four losses
rtol 2e-5 (loss/fraction, a small difference of terms, also atol 1e-6), outgoing priorities rtol
1e-4, the quantile network's Adam parameters rtol 1e-5 / atol 1e-6; the proposal network's
parameters and the RMSprop variant within 4 x what ``fused = False`` deviates on the same GPU
(both optimisers' first steps are sign-like where a gradient is near zero)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import test_fqf_host as fh
from tianshou_amd import _C
from tianshou_amd.policy import FQFPolicy
from tianshou_amd.policy.fqf import _FQFFractionLoss, fqf_select, fraction_loss_kernel
from tianshou_amd.utils.net import (FractionProposalNetwork, FullQuantileFunction, Net,
                                    _FQFProposeFn)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "fqf.npz"))


def _dev_of(got, ref64):
    scale = float(ref64.abs().max()) or 1.0
    return float((got.detach().double() - ref64).abs().max()) / scale


def _ulp(x32):
    ax = x32.abs()
    return torch.nextafter(ax, torch.full_like(ax, float("inf"))) - ax


def _within(name, got, ref64, torch32, what):
    """The 4 x bound of one output; returns the two deviations."""
    k, t = _dev_of(got, ref64), _dev_of(torch32, ref64)
    print(f"{what} {name}: kernel {k:.3g} torch f32 {t:.3g}")
    assert k <= 4 * t, (what, name, k, t)
    return k, t


# -- propose ---------------------------------------------------------------------------------------
PROP_BS = (1, 3, 65)
PROP_NS = (2, 3, 8, 63, 64, 65, 256, 257, 1000, 4096)


def propose_kernel(logits):
    return _FQFProposeFn.apply(logits)


@pytest.mark.parametrize("scale", (1.0, 30.0))
@pytest.mark.parametrize("N", PROP_NS)
@pytest.mark.parametrize("b", PROP_BS)
def test_propose_matches_f64(dev, b, N, scale):
    g = torch.Generator().manual_seed(1000 * b + N + int(scale))
    logits = (scale * torch.randn(b, N, generator=g)).to(dev)
    taus, tau_hats, ent, logp = propose_kernel(logits)
    # the f64 composition on the CPU: its cumsum is sequential
    ref = tuple(t.to(dev) for t in fh.propose_reference(logits.cpu().double()))
    t32 = fh.propose_reference(logits)
    what = f"propose b {b} N {N} x{scale:g}"
    worst = ((taus - ref[0].float()).abs() / _ulp(ref[0].float().clamp(min=1e-30))).max().item()
    on_gpu = fh.propose_reference(logits.double())[0].float()
    other = ((taus - on_gpu).abs() / _ulp(on_gpu.clamp(min=1e-30))).max().item()
    print(f"{what}: taus at most {worst:.2f} ulp from the rounded f64 prefix sums "
          f"({other:.2f} from the same composition run on the GPU)")
    for name, got, r, t in zip(("taus", "tau_hats", "entropies", "logp"),
                               (taus, tau_hats, ent, logp), ref, t32):
        fin = torch.isfinite(r)
        assert torch.equal(torch.isfinite(got), fin), (what, name)
        _within(name, got[fin], r[fin], t[fin], what)
    assert taus.shape == (b, N + 1) and tau_hats.shape == (b, N) and ent.shape == (b,)
    assert bool((taus[:, 0] == 0).all())
    assert bool((taus[:, 1:] >= taus[:, :-1]).all())
    assert torch.equal(tau_hats, (taus[:, :-1] + taus[:, 1:]) / 2.0)


def test_propose_constructed_rows(dev):
    for N in (2, 8, 65, 300, 4096):
        logits = torch.randn(6, N, generator=torch.Generator().manual_seed(N)).to(dev)
        logits[0] = 1.25                       # all equal: taus = i / N, entropy log N
        logits[1, N // 2] = float("-inf")      # a zero-width interval
        logits[3, N - 1] = float("nan")        # a NaN row; its neighbours stay clean
        logits[4, 0] = 80.0                    # one fraction takes nearly everything
        taus, tau_hats, ent, logp = propose_kernel(logits)
        ref = fh.propose_reference(logits.double())
        t32 = fh.propose_reference(logits)
        what = f"constructed N {N}"
        want = torch.arange(N + 1, device=dev, dtype=torch.float64) / N
        # at a power-of-two N torch's f32 leg is exact; half an f32 ulp of 1 is the format's floor
        assert _dev_of(taus[0], want) <= 4 * max(_dev_of(t32[0][0], want), 2.0 ** -24), what
        torch.testing.assert_close(ent[0].double(), torch.log(torch.tensor(
            float(N), dtype=torch.float64, device=dev)), rtol=1e-6, atol=0)
        k = N // 2
        assert taus[1, k] == taus[1, k + 1] and logp[1, k] == float("-inf")
        assert bool(torch.isfinite(ent[1])) and bool(torch.isfinite(taus[1]).all())
        assert taus[3, 0] == 0 and bool(taus[3, 1:].isnan().all())
        assert bool(tau_hats[3].isnan().all()) and bool(ent[3].isnan()) and \
            bool(logp[3].isnan().all())
        keep = [0, 1, 2, 4, 5]
        for name, got, r, t in zip(("taus", "tau_hats", "entropies"), (taus, tau_hats, ent),
                                   ref, t32):
            assert bool(torch.isfinite(got[keep]).all()), (what, name)
            _within(name, got[keep], r[keep], t[keep], what)
        assert bool((taus[keep][:, 1:] >= taus[keep][:, :-1]).all())
        assert torch.equal(tau_hats[keep], ((taus[:, :-1] + taus[:, 1:]) / 2.0)[keep])


@pytest.mark.parametrize("N", PROP_NS[:8])
@pytest.mark.parametrize("b", PROP_BS)
def test_propose_backward_matches_f64_autograd(dev, b, N):
    g = torch.Generator().manual_seed(77 * b + N)
    logits = (3.0 * torch.randn(b, N, generator=g)).to(dev)
    w_taus = torch.randn(b, N + 1, generator=g).to(dev)
    w_ent = torch.randn(b, generator=g).to(dev)

    def grad_of(fn, x, wt, we):
        x = x.detach().clone().requires_grad_(True)
        out = fn(x)
        ((out[0] * wt).sum() + (out[2] * we).sum()).backward()
        return x.grad

    ref = grad_of(fh.propose_reference, logits.double(), w_taus.double(), w_ent.double())
    t32 = grad_of(fh.propose_reference, logits, w_taus, w_ent)
    got = grad_of(propose_kernel, logits, w_taus, w_ent)
    _within("g_logits", got, ref, t32, f"propose backward b {b} N {N}")
    # each incoming gradient alone, and none for the detached midpoints
    x = logits.clone().requires_grad_(True)
    out = propose_kernel(x)
    assert not out[1].requires_grad and not out[3].requires_grad
    (out[2] * w_ent).sum().backward()
    x64 = logits.double().requires_grad_(True)
    (fh.propose_reference(x64)[2] * w_ent.double()).sum().backward()
    assert _dev_of(x.grad, x64.grad) <= 1e-5


def test_propose_argument_errors_and_empty_batch(dev):
    L, s = _C.lib(), _C.stream_ptr(dev)
    for N in (1, _C.DIST_MAX_N + 1):
        logits = torch.zeros(2, N, device=dev)
        outs = [torch.full(shape, 7.0, device=dev) for shape in ((2, N + 1), (2, N), (2,), (2, N))]
        rc = L.tsrl_fqf_propose_fwd(_C.ptr(logits), 2, N, *(_C.ptr(o) for o in outs), s)
        assert rc != 0 and all(bool((o == 7.0).all()) for o in outs), N
        with pytest.raises(_C.TsrlError):
            propose_kernel(logits)
    logits = torch.zeros(2, 4, device=dev)
    outs = [torch.full(shape, 7.0, device=dev) for shape in ((2, 5), (2, 4), (2,), (2, 4))]
    rc = L.tsrl_fqf_propose_fwd(_C.ptr(logits), 2, 4, _C.ptr(outs[0]), _C.ptr(outs[1]), None,
                                _C.ptr(outs[3]), s)
    assert rc != 0 and all(bool((o == 7.0).all()) for o in outs)
    assert L.tsrl_fqf_propose_fwd(None, 0, 4, None, None, None, None, s) == 0
    empty = propose_kernel(torch.zeros(0, 4, device=dev))
    assert [tuple(t.shape) for t in empty] == [(0, 5), (0, 4), (0,), (0, 4)]


def test_module_takes_the_kernel_on_the_device_only(dev):
    torch.manual_seed(3)
    net = FractionProposalNetwork(8, 16).to(dev)
    x = torch.randn(5, 16, device=dev)
    taus, tau_hats, ent = net(x)
    assert type(taus.grad_fn).__name__ == "_FQFProposeFnBackward"
    want = fh.propose_reference(net.net(x).double())
    for got, w in zip((taus, tau_hats, ent), want):
        assert _dev_of(got, w.detach()) <= 1e-6
    (taus[:, 1:-1].sum() - 0.5 * ent.sum()).backward()
    got_w, got_b = net.net.weight.grad.clone(), net.net.bias.grad.clone()
    net.zero_grad()
    net.fused = False
    t2, _, e2 = net(x)
    assert "_FQFProposeFn" not in type(t2.grad_fn).__name__
    (t2[:, 1:-1].sum() - 0.5 * e2.sum()).backward()
    torch.testing.assert_close(got_w, net.net.weight.grad, rtol=1e-4, atol=1e-7)
    torch.testing.assert_close(got_b, net.net.bias.grad, rtol=1e-4, atol=1e-7)
    net.fused = True
    assert "_FQFProposeFn" not in type(net.double()(x.double())[0].grad_fn).__name__


# -- select ----------------------------------------------------------------------------------------
SEL_BS = (1, 63, 65)
SEL_AS = (1, 2, 18)
SEL_NS = (2, 8, 33, 200)


def select_inputs(b, A, N):
    """CPU tensors (sel [b, A, N], eval [b, A, N], taus [b, N + 1]) of one case; the fractions
    are torch's f32 composition of random logits."""
    g = torch.Generator().manual_seed(100000 * b + 1000 * A + N)
    sel, ev = torch.randn(b, A, N, generator=g), torch.randn(b, A, N, generator=g)
    return sel, ev, fh.propose_reference(2.0 * torch.randn(b, N, generator=g))[0]


def weighted_q64(sel, taus):
    """fqf.py:103-107 in f64, the interval widths formed in f32 as torch forms them."""
    return ((taus[:, 1:] - taus[:, :-1]).double().unsqueeze(1) * sel.double()).sum(2)


def top2_rel_gap(q64):
    if q64.shape[1] < 2:
        return torch.full((q64.shape[0],), float("inf"), dtype=torch.float64)
    top = q64.topk(2, dim=1)[0]
    return (top[:, 0] - top[:, 1]) / top.abs().max(dim=1)[0]


def layout(t, major, dev):
    """``t`` [b, A, N] on the device, contiguous ("action") or as the transposed view of a
    contiguous [b, N, A] ("quantile"), which is what the network's head returns."""
    t = t.to(dev)
    if major == "action":
        return t.contiguous()
    return t.transpose(1, 2).contiguous().transpose(1, 2)


@pytest.mark.parametrize("major", ("action", "quantile"))
@pytest.mark.parametrize("N", SEL_NS)
@pytest.mark.parametrize("A", SEL_AS)
@pytest.mark.parametrize("b", SEL_BS)
def test_select_matches_f64(dev, b, A, N, major):
    sel, ev, taus = select_inputs(b, A, N)
    q64 = weighted_q64(sel, taus)
    keep = (top2_rel_gap(q64) >= 1e-6).to(dev)
    assert int((~keep).sum()) <= b // 100
    act_ref = torch.as_tensor(q64.numpy().argmax(axis=1), device=dev)
    q32 = ((taus[:, 1:] - taus[:, :-1]).unsqueeze(1) * sel).sum(2)
    sel, ev, taus = layout(sel, major, dev), layout(ev, major, dev), taus.to(dev)
    q, act, row = fqf_select(sel, taus, ev, want_q=True, want_row=True)
    _within("q", q, q64.to(dev), q32.to(dev), f"select b {b} A {A} N {N} {major}")
    assert act.dtype == torch.int64 and torch.equal(act[keep], act_ref[keep])
    assert torch.equal(act, q.max(dim=1)[1])  # torch's argmax of the rounded sums
    rows = torch.arange(b, device=dev)
    assert row.shape == (b, N) and torch.equal(row, ev[rows, act])
    q2, act2, row2 = fqf_select(sel, taus, None, want_row=True)
    assert q2 is None and torch.equal(act2, act) and torch.equal(row2, sel[rows, act])
    other = "quantile" if major == "action" else "action"
    q4, act4, row4 = fqf_select(sel, taus, layout(ev.cpu(), other, dev), want_q=True,
                                want_row=True)
    assert torch.equal(q4, q) and torch.equal(act4, act) and torch.equal(row4, row)


@pytest.mark.parametrize("major", ("action", "quantile"))
def test_select_constructed_ties_and_strides(dev, major):
    b, A, N = 40, 6, 9
    g = torch.Generator().manual_seed(5)
    sel = torch.randn(b, A, N, generator=g)
    sel[0:10, 4] = sel[0:10, 2] = sel[0:10, 1] + 10.0  # ties among the maxima: 2 before 4
    sel[0:10, 1] -= 30.0
    sel[10:20] = 0.25                                   # constant rows: action 0
    sel[20:30, 5] = 50.0                                # the maximum in another wave's action
    taus = fh.propose_reference(torch.randn(b, N, generator=g))[0].to(dev)
    sel = layout(sel, major, dev)
    q, act, row = fqf_select(sel, taus, want_q=True, want_row=True)
    assert act[0:10].tolist() == [2] * 10 and torch.equal(q[0:10, 2], q[0:10, 4])
    assert act[10:20].tolist() == [0] * 10 and act[20:30].tolist() == [5] * 10
    assert torch.equal(act, q.max(dim=1)[1])
    q, act, row = fqf_select(sel[:0], taus[:0], want_q=True, want_row=True)
    assert q.shape == (0, A) and act.shape == (0,) and row.shape == (0, N)
    # foreign strides are refused before any launch
    L = _C.lib()
    x = torch.randn(4, 3, 8, device=dev)
    t4 = fh.propose_reference(torch.randn(4, 4))[0].to(dev)
    out = torch.full((4,), -5, dtype=torch.int64, device=dev)
    rc = L.tsrl_fqf_select(_C.ptr(x), 16, 2, None, 0, 0, _C.ptr(t4), 4, 3, 4, None, _C.ptr(out),
                           None, _C.stream_ptr(dev))
    assert rc != 0 and bool((out == -5).all())
    rc = L.tsrl_fqf_select(_C.ptr(x), 4, 1, _C.ptr(x), 16, 2, _C.ptr(t4), 4, 3, 4, None,
                           _C.ptr(out), None, _C.stream_ptr(dev))
    assert rc != 0 and bool((out == -5).all())


# -- fraction loss ---------------------------------------------------------------------------------
FRAC_AS = (1, 6)
FRAC_NS = (2, 3, 8, 64, 65, 300)


def fraction_inputs(b, A, N):
    """CPU tensors (curr [b, A, N], qtau [b, A, N - 1], act [b]) on the dyadic grid k / 64 in
    [-4, 4]: every subtraction and comparison of fqf.py:147-160 is exact in f32 and f64 alike.
    Every fifth row holds a tie of each sign test in the taken action."""
    g = torch.Generator().manual_seed(7000 * b + 100 * A + N)
    curr = torch.randint(-256, 257, (b, A, N), generator=g).float() / 64
    qtau = torch.randint(-256, 257, (b, A, N - 1), generator=g).float() / 64
    act = torch.randint(0, A, (b,), generator=g)
    for r in range(0, b, 5):
        a = int(act[r])
        qtau[r, a, 0] = curr[r, a, 0]             # q_1 == L_1
        curr[r, a, N - 1] = qtau[r, a, N - 2]     # q_{N-1} == R_{N-1}
    return curr, qtau, act


def tie_counts(hats, q):
    left = torch.cat([hats[:, :1], q[:, :-1]], dim=1)
    right = torch.cat([q[:, 1:], hats[:, -1:]], dim=1)
    return int((q == left).sum()), int((q == right).sum())


@pytest.mark.parametrize("major", ("action", "quantile"))
@pytest.mark.parametrize("N", FRAC_NS)
@pytest.mark.parametrize("A", FRAC_AS)
@pytest.mark.parametrize("b", SEL_BS)
def test_fraction_loss_matches_f64(dev, b, A, N, major):
    curr_c, qtau_c, act_c = fraction_inputs(b, A, N)
    rows_c = torch.arange(b)
    left, right = tie_counts(curr_c[rows_c, act_c], qtau_c[rows_c, act_c])
    assert left > 0 and right > 0
    g = torch.Generator().manual_seed(N + b)
    logits = (2.0 * torch.randn(b, N, generator=g)).to(dev)
    taus, _, ent, logp = propose_kernel(logits)
    curr, qtau, act = layout(curr_c, major, dev), layout(qtau_c, major, dev), act_c.to(dev)
    rows = torch.arange(b, device=dev)
    hats, q = curr[rows, act], qtau[rows, act]
    G32 = fh.gradient_of_taus(hats, q)
    assert torch.equal(G32.double(), fh.gradient_of_taus(hats.double(), q.double()))
    for ent_coef in (0.0, 10.0):
        what = f"fraction b {b} A {A} N {N} {major} ent_coef {ent_coef:g}"
        losses, g_logits, G = fraction_loss_kernel(curr, qtau, act, taus, logp, ent, ent_coef,
                                                   want_grad_taus=True)
        assert torch.equal(G, G32), what
        # the f64 composition on the f32 inputs the kernel reads
        ref_l = torch.stack(((G32.double() * taus.double()[:, 1:-1]).sum(1).mean(),
                             ent.double().mean()))
        t32_l = torch.stack(((G32 * taus[:, 1:-1]).sum(1).mean(), ent.mean()))
        _within("fraction loss", losses[0:1], ref_l[0:1], t32_l[0:1], what)
        _within("entropy loss", losses[1:2], ref_l[1:2], t32_l[1:2], what)
        ref_g = fh.g_logits_formula(G32, logp, ent, ent_coef)
        # f64 autograd and torch's f32 autograd on the reference lines from the same logits
        grads = []
        for x in (logits.double(), logits):
            x = x.detach().clone().requires_grad_(True)
            t_, _, e_, _ = fh.propose_reference(x)
            ((G32.to(x.dtype) * t_[:, 1:-1]).sum(1).mean() - ent_coef * e_.mean()).backward()
            grads.append(x.grad)
        k, t = _within("g_logits", g_logits, grads[0], grads[1], what)
        kc = _dev_of(g_logits, ref_g)
        print(f"{what} g_logits against the f64 composition on its own inputs: {kc:.3g}")
        assert kc <= 4 * t, (what, kc, t)


def test_fraction_loss_edges(dev):
    b, A, N = 7, 3, 2
    # N = 2: the single interior fraction, both neighbours hats
    curr_c, qtau_c, act_c = fraction_inputs(b, A, N)
    curr, qtau, act = curr_c.to(dev), qtau_c.to(dev), act_c.to(dev)
    taus, _, ent, logp = propose_kernel(torch.randn(b, N, device=dev))
    rows = torch.arange(b, device=dev)
    losses, g_logits, G = fraction_loss_kernel(curr, qtau, act, taus, logp, ent, 1.5,
                                               want_grad_taus=True)
    h, q = curr[rows, act], qtau[rows, act]
    v1, v2 = q[:, 0] - h[:, 0], q[:, 0] - h[:, 1]
    want = torch.where(q[:, 0] > h[:, 0], v1, -v1) + torch.where(q[:, 0] < h[:, 1], v2, -v2)
    assert G.shape == (b, 1) and torch.equal(G[:, 0], want)
    assert _dev_of(g_logits, fh.g_logits_formula(G, logp, ent, 1.5)) <= 1e-6
    # an out-of-range action: NaN losses and that row only
    bad = act.clone()
    bad[2] = A
    losses, g_logits, G = fraction_loss_kernel(curr, qtau, bad, taus, logp, ent, 1.5,
                                               want_grad_taus=True)
    assert bool(losses.isnan().all()) and bool(g_logits[2].isnan().all()) and \
        bool(G[2].isnan().all())
    keep = [0, 1, 3, 4, 5, 6]
    assert bool(torch.isfinite(g_logits[keep]).all()) and bool(torch.isfinite(G[keep]).all())
    # a fraction of exactly zero width gets a zero gradient
    logits = torch.randn(b, 8, device=dev)
    logits[:, 3] = float("-inf")
    taus, _, ent, logp = propose_kernel(logits)
    c8, q8, a8 = (t.to(dev) for t in fraction_inputs(b, A, 8))
    _, g_logits, _ = fraction_loss_kernel(c8, q8, a8, taus, logp, ent, 10.0)
    assert bool((g_logits[:, 3] == 0).all()) and bool(torch.isfinite(g_logits).all())
    # argument errors launch nothing
    L, s = _C.lib(), _C.stream_ptr(dev)
    out = torch.full((b, 8), 7.0, device=dev)
    two = torch.full((2,), 7.0, device=dev)
    parts = torch.empty(2 * b, dtype=torch.float64, device=dev)
    for n, sa, sn, ta, tn, part in ((1, 1, 1, 1, 1, parts), (_C.DIST_MAX_N + 1, 8, 1, 7, 1, parts),
                                    (8, 16, 2, 7, 1, parts), (8, 8, 1, 14, 2, parts),
                                    (8, 8, 1, 7, 1, None)):
        rc = L.tsrl_fqf_fraction_loss_fwd_bwd(
            _C.ptr(c8), sa, sn, _C.ptr(q8), ta, tn, _C.ptr(a8), _C.ptr(taus), _C.ptr(logp),
            _C.ptr(ent), 1.0, b, A, n, _C.ptr(out), None, _C.ptr(part), _C.ptr(two), s)
        assert rc != 0 and bool((out == 7.0).all()) and bool((two == 7.0).all()), n
    # b == 1 needs no partials
    losses, g1, _ = fraction_loss_kernel(c8[:1], q8[:1], a8[:1], taus[:1], logp[:1], ent[:1], 10.0)
    G1 = fh.gradient_of_taus(c8[:1][[0], a8[:1]], q8[:1][[0], a8[:1]])
    assert _dev_of(g1, fh.g_logits_formula(G1, logp[:1], ent[:1], 10.0)) <= 1e-6
    assert losses[1] == ent[0]


def test_fraction_loss_seed_paths_and_static_outputs(dev):
    from tianshou_amd.policy.onpolicy import _unit_seed
    b, A, N = 65, 6, 8
    curr, qtau, act = (t.to(dev) for t in fraction_inputs(b, A, N))
    curr = layout(curr, "quantile", dev)
    logits = torch.randn(b, N, device=dev)
    grads = []
    for seed in ("ones", "unit", 2.5):
        x = logits.clone().requires_grad_(True)
        taus, _, ent, logp = propose_kernel(x)
        handle, losses = _FQFFractionLoss.apply(x, taus.detach(), ent,
                                                (curr, qtau, act, logp, 10.0, None))
        assert not losses.requires_grad
        torch.testing.assert_close(handle.detach(), losses[0] - 10.0 * losses[1], rtol=1e-6,
                                   atol=0)
        if seed == "ones":
            handle.backward()
        elif seed == "unit":
            handle.backward(_unit_seed(dev))
        else:
            (handle * seed).backward()
        grads.append(x.grad.clone())
    assert torch.equal(grads[0], grads[1])
    torch.testing.assert_close(grads[2], 2.5 * grads[0], rtol=1e-6, atol=0)
    out = torch.full((4,), 7.0, device=dev)
    x = logits.clone().requires_grad_(True)
    taus, _, ent, logp = propose_kernel(x)
    handle, losses = _FQFFractionLoss.apply(x, taus.detach(), ent,
                                            (curr, qtau, act, logp, 10.0, out))
    assert out[0] == 7.0 and losses.data_ptr() == out[1:3].data_ptr()
    assert out[3] == handle.detach()
    torch.testing.assert_close(out[3], out[1] - 10.0 * out[2], rtol=1e-6, atol=0)
    # a foreign proposal: taus and entropies get gradient_of_taus / b and -ent_coef / b
    x = logits.clone().requires_grad_(True)
    t_, _, e_, _ = fh.propose_reference(x)
    handle, _ = _FQFFractionLoss.apply(None, t_, e_, (curr, qtau, act, None, 10.0, None))
    handle.backward()
    assert _dev_of(x.grad, grads[0].double()) <= 1e-5


# -- update() against the recording ----------------------------------------------------------------
from tests import test_gpu_dqn as gd  # noqa: E402  (its buffer / recorder helpers)

TAGS = fh.TAGS
ADAM_TAGS = ("target", "notarget", "uneven", "per")
LEGS = {"graph": dict(fused=True, graph_learn=True), "eager": dict(fused=True, graph_learn=False),
        "torch": dict(fused=False)}


_FRACTION_APPLY = _FQFFractionLoss.apply


def _cfg(z):
    return json.loads(str(z["learn_cfg"]))


def _spy_quantiles(policy, seen):
    """Record the taken action's sa_quantile_hats / sa_quantiles of every update: the fused
    legs' from the fraction loss's inputs, the torch leg's from learn()'s own forward."""
    apply, forward = _FRACTION_APPLY, policy.forward

    def pick(logits, quantiles_tau, act):
        rows = torch.arange(len(act), device=logits.device)
        act = torch.as_tensor(act, device=logits.device).long()
        seen.append((logits.detach()[rows, act].clone(), quantiles_tau.detach()[rows, act].clone()))

    def spy_apply(logits, taus, ent, args):
        pick(args[0], args[1], args[2])
        return apply(logits, taus, ent, args)

    def spy_forward(batch, *a, **kw):
        res = forward(batch, *a, **kw)
        if not policy.fused and kw.get("input", "obs") == "obs":
            pick(res.logits, res.quantiles_tau, batch.act)
        return res

    policy.forward = spy_forward
    return spy_apply


def _run_variant(z, dev, tag, check_params, monkeypatch, **attrs):
    from tianshou_amd.policy import fqf as fqf_mod
    cfg = _cfg(z)
    policy, v = fh.make_policy(z, cfg, tag, dev, **attrs)
    buf = gd._filled_buffer(z, cfg, dev, per=bool(v.get("per")))
    seen = gd._record(policy)
    quantiles = []
    spy = _spy_quantiles(policy, quantiles)
    monkeypatch.setattr(fqf_mod._FQFFractionLoss, "apply", spy, raising=False)
    np.random.seed(v["seed"])
    margin = float(z[tag + "_min_margin"])
    for u in range(cfg["updates"]):
        del quantiles[:]
        res = policy.update(v["bs"], buf)
        q = f"{tag}_u{u}_"
        s = seen[u]
        assert s["indices"].tolist() == z[q + "indices"].tolist(), q
        # a replayed graph launches no Python: its quantiles are checked through the eager leg,
        # whose update it equals bit for bit (test_graph_replay_is_bitwise_eager)
        assert len(quantiles) == (0 if policy._learn_graphs and u > 1 else 1), q
        for hats, sq in quantiles:
            d = max(np.abs(hats.cpu().numpy() - z[q + "sa_quantile_hats"]).max(),
                    np.abs(sq.cpu().numpy() - z[q + "sa_quantiles"]).max())
            print(f"{q} sa quantiles deviate {d:.3g}, half the recorded margin {margin / 2:.3g}")
            assert d < margin / 2, (q, d, margin)
        out_w = s["td_error"]  # the recorder's name for the outgoing batch.weight
        print(f"{q} " + " ".join(f"{k} {res[k]:.7g} ({float(z[q + k.replace('/', '_')]):.7g})"
                                 for k in fh.LOSS_KEYS)
              + f" max|dparam| {gd._param_dev(policy.model, z, q + 'param_'):.3g} proposal "
              f"{gd._param_dev(policy.propose_model, z, q + 'pparam_'):.3g}")
        np.testing.assert_allclose(s["returns"].cpu().numpy(), z[q + "returns"], rtol=1e-5,
                                   atol=1e-6, err_msg=q)
        assert tuple(res) == fh.LOSS_KEYS
        for k in fh.LOSS_KEYS:
            np.testing.assert_allclose(res[k], float(z[q + k.replace("/", "_")]), rtol=2e-5,
                                       atol=1e-6 if k == "loss/fraction" else 0, err_msg=q + k)
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


def _proposal_dev(z, tag, into):
    return lambda u, p: into.append(gd._param_dev(p.propose_model, z, f"{tag}_u{u}_pparam_"))


@pytest.mark.parametrize("tag", ADAM_TAGS)
def test_update_matches_reference_adam(z, dev, tag, monkeypatch):
    """The quantile network's parameters at Adam's tolerance on every leg; the proposal
    network's within 4 x the torch leg's deviation."""
    devs = {}
    for leg in ("torch", "graph", "eager"):
        devs[leg] = []

        def check(u, policy, leg=leg):
            for k, t in policy.model.state_dict().items():
                np.testing.assert_allclose(t.cpu().numpy(), z[f"{tag}_u{u}_param_{k}"],
                                           rtol=1e-5, atol=1e-6,
                                           err_msg=f"{tag} {leg} update {u} {k}")
            _proposal_dev(z, tag, devs[leg])(u, policy)

        policy = _run_variant(z, dev, tag, check, monkeypatch, **LEGS[leg])
        if leg == "torch":
            assert policy._flat is None and policy._frac_flat is None
            assert not policy._learn_graphs
            continue
        assert policy._flat.adam_bound(policy.optim)
        assert policy._frac_flat.adam_bound(policy._fraction_optim)
        assert not policy._graph_failed
        assert len(policy._learn_graphs) == (1 if leg == "graph" else 0)
        print(f"{tag} proposal max|dparam| per update: torch {devs['torch']} {leg} {devs[leg]}")
        for u, (f, t) in enumerate(zip(devs[leg], devs["torch"])):
            assert f <= 4 * t, (tag, leg, u, f, t)


def test_update_matches_reference_rmsprop(z, dev, monkeypatch):
    """Both networks' max |parameter - recorded| after each update stays within 4 x the torch
    formulation's on the same GPU (all printed)."""
    def both(into):
        return lambda u, p: into.append((gd._param_dev(p.model, z, f"rms_u{u}_param_"),
                                         gd._param_dev(p.propose_model, z, f"rms_u{u}_pparam_")))
    torch_dev = []
    _run_variant(z, dev, "rms", both(torch_dev), monkeypatch, **LEGS["torch"])
    for leg in ("graph", "eager"):
        fused_dev = []
        policy = _run_variant(z, dev, "rms", both(fused_dev), monkeypatch, **LEGS[leg])
        print("rms max|dparam| (model, proposal) per update: torch", torch_dev, leg, fused_dev)
        assert policy._flat.adam_bound(policy.optim)
        assert policy._frac_flat.adam_bound(policy._fraction_optim)
        assert bool(policy._learn_graphs) == (leg == "graph")
        for u in range(len(torch_dev)):
            for f, t in zip(fused_dev[u], torch_dev[u]):
                assert f <= 4 * t, (leg, u, fused_dev[u], torch_dev[u])


def _updates(z, dev, tag, **attrs):
    cfg = _cfg(z)
    policy, v = fh.make_policy(z, cfg, tag, dev, fused=True, **attrs)
    buf = gd._filled_buffer(z, cfg, dev, per=bool(v.get("per")))
    np.random.seed(v["seed"])
    out = []
    for u in range(cfg["updates"]):
        res = policy.update(v["bs"], buf)
        out.append((res, [p.detach().clone() for p in policy.model.parameters()] +
                    [p.detach().clone() for p in policy.propose_model.parameters()]))
    return policy, out


@pytest.mark.parametrize("tag", TAGS)
def test_graph_replay_is_bitwise_eager(z, dev, tag):
    pol_g, out_g = _updates(z, dev, tag, graph_learn=True)
    pol_e, out_e = _updates(z, dev, tag, graph_learn=False)
    assert len(pol_g._learn_graphs) == 1 and not pol_e._learn_graphs
    for (res_g, par_g), (res_e, par_e) in zip(out_g, out_e):
        assert res_g == res_e and tuple(res_g) == fh.LOSS_KEYS
        assert len(par_g) == len(par_e) > 2
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
    assert len({res["loss"] for res, _ in out}) == len(out)  # the replays saw fresh rows


# -- other paths -----------------------------------------------------------------------------------
def test_reference_checkpoint_loads_strict_and_gives_the_recorded_loss(z, dev, tmp_path):
    cfg = _cfg(z)
    v, n = cfg["variants"]["target"], cfg["net"]
    paths = [os.path.join(tmp_path, name) for name in ("fqf_model.pth", "fqf_propose.pth")]
    torch.save(fh.init_state(z), paths[0])
    torch.save(fh.init_state(z, "target_pinit_"), paths[1])
    torch.manual_seed(99)  # other initial weights than the checkpoints'
    feature = Net(cfg["D"], n["feature_out"], hidden_sizes=n["feature_hidden"], device=dev)
    net = FullQuantileFunction(feature, cfg["A"], hidden_sizes=n["head_hidden"],
                               num_cosines=n["num_cosines"], device=dev).to(dev)
    propose = FractionProposalNetwork(v["N"], net.input_dim).to(dev)
    assert list(net.state_dict()) == json.loads(str(z["state_keys"]))
    for module, path in zip((net, propose), paths):
        res = module.load_state_dict(torch.load(path, map_location=dev), strict=True)
        assert not res.missing_keys and not res.unexpected_keys
    optim, frac_optim = fh.make_optims(v, cfg, net, propose)
    policy = FQFPolicy(net, optim, propose, frac_optim, discount_factor=cfg["gamma"],
                       num_fractions=v["N"], ent_coef=v["ent_coef"],
                       estimation_step=v["n_step"], target_update_freq=v["freq"]).to(dev)
    policy.train()
    buf = gd._filled_buffer(z, cfg, dev)
    np.random.seed(v["seed"])
    res = policy.update(v["bs"], buf)
    for k in fh.LOSS_KEYS:
        np.testing.assert_allclose(res[k], float(z["target_u0_" + k.replace("/", "_")]),
                                   rtol=2e-5, atol=1e-6 if k == "loss/fraction" else 0)


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


def test_fused_false_launches_none_of_the_kernels(z, dev, monkeypatch):
    """``policy.fused = False`` is the reference's op sequence throughout: no tsrl_fqf_* call, no
    embedding kernel in either network's graph, no proposal kernel; all back with True."""
    from tianshou_amd.data import Batch
    policy, v = fh.make_policy(z, _cfg(z), "target", dev)
    obs = torch.as_tensor(z["add_obs"][:9]).to(dev)
    batch = Batch(obs=obs, obs_next=obs, info=Batch())
    res = policy(batch)
    assert "_IQNEmbedFnBackward" in _graph_nodes(res.logits)
    assert {"_FQFProposeFnBackward", "_LinearFnBackward"} <= _graph_nodes(res.fractions.taus)
    policy.fused = False
    called = []
    lib = _C.lib()

    class Spy:
        def __getattr__(self, name):
            if name.startswith(("tsrl_fqf_", "tsrl_iqn_")):
                called.append(name)
            return getattr(lib, name)

    monkeypatch.setattr(_C, "lib", lambda: Spy())
    for model in ("model", "model_old"):
        for p in getattr(policy, model).parameters():
            p.requires_grad_(True)
        res = policy(batch, model=model)
        nodes = _graph_nodes(res.logits) | _graph_nodes(res.fractions.taus)
        assert not {"_IQNEmbedFnBackward", "_FQFProposeFnBackward"} & nodes
        assert "AddmmBackward0" in nodes
    rows = policy._next_rows(batch)
    out = policy.learn(Batch(obs=obs, act=torch.zeros(9, dtype=torch.int64, device=dev),
                             returns=rows, info=Batch()))
    assert tuple(out) == fh.LOSS_KEYS and not called
    assert policy._flat is None and policy._frac_flat is None
    policy.fused = True
    res = policy(batch)
    assert "_IQNEmbedFnBackward" in _graph_nodes(res.logits)
    assert "tsrl_fqf_select" in called and "tsrl_fqf_propose_fwd" in called


@pytest.mark.parametrize("tag", ("target", "notarget"))
def test_target_q_equals_the_reference_shaped_path(z, dev, tag):
    """``_target_q`` skips the quantiles_tau pass of fqf.py:61-74; on the torch leg its rows are
    bitwise those of the reference-shaped calls that compute it, and the fused leg's agree."""
    from tianshou_amd.data import Batch
    cfg = _cfg(z)
    policy, v = fh.make_policy(z, cfg, tag, dev, fused=False)
    buf = gd._filled_buffer(z, cfg, dev)
    idx = z[f"{tag}_u0_indices"]
    got = policy._target_q(buf, idx)
    with torch.no_grad():
        batch = Batch(obs_next=buf.get(idx, "obs_next"), info=Batch())
        result = policy(batch, input="obs_next")
        assert result.quantiles_tau is not None
        next_dist = policy(batch, model="model_old", input="obs_next",
                           fractions=result.fractions).logits if policy._target \
            else result.logits
        want = next_dist[torch.arange(len(idx), device=dev), result.act, :]
    assert torch.equal(got, want)
    policy.fused = True
    fused = policy._target_q(buf, idx)
    torch.testing.assert_close(fused, want, rtol=1e-5, atol=1e-6)


def test_collector_writes_the_same_rows_with_step_capture_on_and_off(dev):
    from tianshou_amd.data import Collector, VectorReplayBuffer
    from tianshou_amd.env import SyntheticVectorEnv
    E, T, D, A = 8, 40, 12, 6
    rows = {}
    for graph_steps in (True, False):
        torch.manual_seed(0)
        np.random.seed(0)
        env = SyntheticVectorEnv(E, (D,), A, ep_len=10, device=dev, discrete=True)
        feature = Net(D, 16, hidden_sizes=(16,), device=dev)
        net = FullQuantileFunction(feature, A, hidden_sizes=(16,), num_cosines=16,
                                   device=dev).to(dev)
        propose = FractionProposalNetwork(8, net.input_dim).to(dev)
        policy = FQFPolicy(net, torch.optim.Adam(net.parameters(), lr=1e-3), propose,
                           torch.optim.Adam(propose.parameters(), lr=1e-3), num_fractions=8,
                           target_update_freq=4, action_space=env.action_space).to(dev)
        assert not getattr(policy, "eager_collect_step", False)
        policy.eval()
        policy.set_eps(0.0)
        buf = VectorReplayBuffer(E * T * 2, E, device=dev)
        col = Collector(policy, env, buf)
        if not graph_steps:
            col.graph_steps = 0
        res = col.collect(n_step=E * T)
        assert res["n/st"] == E * T and len(buf) == E * T
        assert bool(col._graphs) == graph_steps  # the step was captured, or never
        batch, _ = buf.sample(0)
        rows[graph_steps] = {k: torch.as_tensor(batch[k]).clone()
                             for k in ("obs", "act", "rew", "terminated", "truncated",
                                       "obs_next")}
    for k, t in rows[True].items():
        assert torch.equal(t, rows[False][k]), k
