"""csrc/ensemble.hip through the C ABI and through utils.net.ensemble_critic, and REDQPolicy's
target with ``fused_ensemble`` on / off.

Bound (tests/test_gpu_gail.py's): max-abs and 2-norm error against the f64 restatement
(tests/ensemble_common.py) at most 4 x the error of the same formulation in f32 on the CPU on
identical inputs, floor 2^-23 of the reference's norm.  Outputs sit between NaN guard bands.  Each
test prints its measured ratio."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ensemble_common as ec
from tianshou_amd import _C

pytestmark = pytest.mark.gpu
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _guarded(shape, dev):
    n = int(np.prod(shape))
    t = torch.full((n + 2 * GUARD,), float("nan"), device=dev)
    return t, t[GUARD:GUARD + n].view(shape)


def _intact(full):
    return bool(full[:GUARD].isnan().all() and full[-GUARD:].isnan().all())


def _inputs(case, dev):
    """The case on the device: obs / act as views with pitches larger than their widths."""
    b, D, A, H, E = case
    params, obs, act = ec.make(*case)
    pitched = []
    for x, pad in ((obs, 3), (act, 32)):
        pitched.append(torch.zeros(b, x.shape[1] + pad, device=dev)[:, :x.shape[1]])
        pitched[-1].copy_(x.float())
    w = [p.float().contiguous().to(dev) for p in params]
    args = (pitched[0].data_ptr(), D + 3, pitched[1].data_ptr(), A + 32, b, D, A, H, E)
    return (params, obs, act), args, _C.EnsNet(*(t.data_ptr() for t in w)), [pitched, w]


def _fwd(args, net, dev, members=None):
    """(rc, q [S or E, b]) of one tsrl_ens_critic_fwd call, the guard bands checked."""
    b, E = args[4], args[8]
    host = None if members is None else np.asarray(members, dtype=np.int32)
    idx = None if host is None else torch.as_tensor(host, device=dev)
    full, q = _guarded((E if host is None else min(len(host), E), b), dev)
    rc = _C.lib().tsrl_ens_critic_fwd(
        *args, ctypes.byref(net), None if idx is None else idx.data_ptr(),
        None if host is None else host.ctypes.data, 0 if host is None else len(host),
        q.data_ptr(), None)
    torch.cuda.synchronize(dev)
    assert _intact(full)
    return rc, q


@pytest.mark.parametrize("case", ec.CASES + [ec.WALK], ids=str)
def test_forward_matches_f64(dev, case):
    ref, args, net, _keep = _inputs(case, dev)
    rc, q = _fwd(args, net, dev)
    _C.check(rc, "fwd")
    assert torch.equal(q, _fwd(args, net, dev)[1])  # a second call is bitwise equal
    worst = ec.worst_ratio(q.cpu(), ec.forward(*ref, torch.float32), ec.forward(*ref))
    print(f"forward {case}: worst error ratio to f32 {worst:.3f}")
    assert worst <= 4.0


def test_members_are_rows_of_the_full_result(dev):
    case = ec.CASES[2]  # E = 3
    _, args, net, _keep = _inputs(case, dev)
    full = _fwd(args, net, dev)[1]
    rc, sub = _fwd(args, net, dev, members=(2, 0))
    _C.check(rc, "fwd")
    assert torch.equal(sub, full[[2, 0]])
    for bad in ((0, 3), (-1,), (0, 1, 2, 0)):  # outside [0, E); S > E
        rc, q = _fwd(args, net, dev, members=bad)
        assert rc != 0 and rc != _C.ERR_ENS_SHAPE and bool(q.isnan().all())
        assert b"tsrl_ens_critic_fwd" in _C.lib().tsrl_last_error()
    for i, v in ((7, 64), (5, 510), (8, 65)):  # H, D + A = 513, E the kernel declines
        rc, q = _fwd(args[:i] + (v,) + args[i + 1:], net, dev)
        assert rc == _C.ERR_ENS_SHAPE and bool(q.isnan().all())


def _count_members(monkeypatch):
    """The S argument of every tsrl_ens_critic_fwd call from here on."""
    calls, fn = [], _C.lib().tsrl_ens_critic_fwd
    monkeypatch.setattr(_C.lib(), "tsrl_ens_critic_fwd",
                        lambda *a: (calls.append(a[12]), fn(*a))[1])
    return calls


def test_ensemble_critic_dispatch(dev, monkeypatch):
    """The Python entry: the C ABI's bits where the critic matches; the torch lines' bits for a
    width the kernel declines, another activation and a recorded gradient."""
    from tianshou_amd.utils.net import ensemble_critic
    torch.manual_seed(3)
    obs, act = torch.randn(33, ec.D, device=dev), torch.randn(33, ec.A, device=dev)
    critic = ec.make_critics(dev)
    w = [p.detach() for p in critic.parameters()]  # w1, b1, w2, b2, w3, b3
    args = (obs.data_ptr(), ec.D, act.data_ptr(), ec.A, 33, ec.D, ec.A, ec.HIDDEN[0], ec.MEMBERS)
    want = _fwd(args, _C.EnsNet(*(t.data_ptr() for t in w)), dev)[1]
    calls = _count_members(monkeypatch)
    with torch.no_grad():
        assert torch.equal(ensemble_critic(critic, obs, act), want.unsqueeze(-1))
        assert torch.equal(ensemble_critic(critic, obs, act, members=[2, 0]),
                           want[[2, 0]].unsqueeze(-1))
        torch_q = critic(obs, act)
        assert torch.equal(ensemble_critic(critic, obs, act, fused=False), torch_q)
        for other in (ec.make_critics(dev, hidden=(16, 16)),
                      ec.make_critics(dev, activation=torch.nn.Tanh)):
            assert torch.equal(ensemble_critic(other, obs, act), other(obs, act))
            assert torch.equal(ensemble_critic(other, obs, act, members=[2, 0]),
                               other(obs, act)[[2, 0]])
    q = ensemble_critic(critic, obs, act.requires_grad_())  # grad mode: the torch lines
    assert q.requires_grad and torch.equal(q.detach(), torch_q)
    assert calls == [0, 2]  # nothing but the matching critic under no_grad reached the library


def test_redq_target_evaluates_the_subset_only(dev, monkeypatch):
    """Two updates (a critic-only one, then one that steps the actor) with fused_ensemble on
    against off from identical states and draws: returns and losses to rtol 1e-5, parameter
    deltas to rtol 1e-4 / atol 1e-6 max|delta| (tests/test_gpu_redq.py's q-loss gradient bound);
    the on leg's target forward computed SUBSET members, the off leg called no ensemble kernel."""
    runs, calls = {}, _count_members(monkeypatch)
    for on in (True, False):
        policy, buf = ec.make_policy(dev, on)
        assert policy.fused_ensemble is on
        before = torch.cat([p.detach().reshape(-1) for p in policy.parameters()]).clone()
        process_fn, returns = policy.process_fn, []
        policy.process_fn = lambda *a: (lambda bt: (returns.append(bt.returns.clone()), bt)[1])(
            process_fn(*a))
        np.random.seed(ec.SEED)
        torch.manual_seed(ec.SEED)
        calls.clear()
        res = [policy.update(ec.BATCH, buf) for _ in range(2)]
        assert calls == ([ec.SUBSET] * 2 if on else [])
        after = torch.cat([p.detach().reshape(-1) for p in policy.parameters()])
        runs[on] = (res, torch.stack(returns).cpu().double(), (after - before).cpu().double())
    (r1, ret1, d1), (r0, ret0, d0) = runs[True], runs[False]
    assert [sorted(r) for r in r1] == [sorted(r) for r in r0] and "loss/actor" in r1[1]
    print(f"redq on / off: returns max rel {float(((ret1 - ret0) / ret0).abs().max()):.3g}, "
          f"deltas max abs {float((d1 - d0).abs().max()):.3g} of {float(d0.abs().max()):.3g}")
    for a, c in zip(r1, r0):
        np.testing.assert_allclose([a[k] for k in sorted(a)], [c[k] for k in sorted(c)], rtol=1e-5)
    np.testing.assert_allclose(ret1, ret0, rtol=1e-5)
    assert float(d0.abs().max()) > 0
    np.testing.assert_allclose(d1, d0, rtol=1e-4, atol=1e-6 * float(d0.abs().max()))
