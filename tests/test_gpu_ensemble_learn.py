"""The training path of csrc/ensemble.hip: tsrl_ens_critic_fwd_save / tsrl_ens_critic_bwd through
the C ABI, through utils.net.ensemble_critic(learn=True), and REDQPolicy with
``fused_ensemble_learn`` on / off.

Reference: tests/ensemble_common.py's f64 forward under torch.autograd.grad with a seeded dq.
Bound (tests/test_gpu_ensemble.py's): max-abs and 2-norm error of each output block at most 4 x
the error of the same formulation in f32 on the CPU, floor 2^-23 of the reference's norm.  A
gradient bound means nothing where a pre-activation sits on the ReLU kink, so each case uses the
first seed at which, on the CPU alone, the f32 masks equal the f64 masks and the smallest f64
|pre-activation| exceeds 16 x the largest f32-vs-f64 pre-activation error.  Worst measured ratios:
profiles/ensemble_learn_gpu_tests.log."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import ensemble_common as ec
from tianshou_amd import _C

pytestmark = pytest.mark.gpu
NAMES = ("dw1", "db1", "dw2", "db2", "dw3", "db3", "da")
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _guarded(shape, dev):
    """(the whole buffer, its view of ``shape``) between two NaN guard bands."""
    n = int(np.prod(shape))
    t = torch.full((n + 2 * GUARD,), float("nan"), device=dev)
    return t, t[GUARD:GUARD + n].view(shape)


def _intact(full):
    return bool(full[:GUARD].isnan().all() and full[-GUARD:].isnan().all())


def _fwd(args, net, dev):
    """q [E, b] of the plain forward tsrl_ens_critic_fwd over all members."""
    full, q = _guarded((args[8], args[4]), dev)
    _C.check(_C.lib().tsrl_ens_critic_fwd(*args, ctypes.byref(net), None, None, 0, q.data_ptr(),
                                          None), "tsrl_ens_critic_fwd")
    torch.cuda.synchronize(dev)
    assert _intact(full)
    return q


def _pre(params, obs, act, dtype):
    w1, b1, w2, b2 = (p.to(dtype) for p in params[:4])
    z1 = torch.matmul(torch.cat([obs, act], 1).to(dtype), w1) + b1
    return torch.cat([z1.reshape(-1), (torch.matmul(torch.relu(z1), w2) + b2).reshape(-1)]).double()


def _grads(params, obs, act, dq, dtype):
    leaves = [p.to(dtype).requires_grad_() for p in params] + [act.to(dtype).requires_grad_()]
    return torch.autograd.grad(ec.forward(leaves[:6], obs, leaves[6], dtype), leaves, dq.to(dtype))


@functools.lru_cache(None)
def _reference(case):
    """(seed, ReLU condition, dq, f32 gradients, f64 gradients), computed once per case."""
    for seed in range(64):
        params, obs, act = ec.make(*case, seed=seed)
        z64, z32 = _pre(params, obs, act, torch.float64), _pre(params, obs, act, torch.float32)
        cond = (bool(((z64 > 0) == (z32 > 0)).all()), float(z64.abs().min()),
                float((z32 - z64).abs().max()))
        if cond[0] and cond[1] > 16 * cond[2]:
            break
    dq = torch.randn(case[4], case[0], generator=torch.Generator().manual_seed(seed)).double()
    return seed, cond, dq, _grads(params, obs, act, dq, torch.float32), \
        _grads(params, obs, act, dq, torch.float64)


def _case(case, dev):
    """The case on the device at its chosen seed, obs / act as views with pitches larger than
    their widths: (args, net, keep-alive)."""
    b, D, A, H, E = case
    params, obs, act = ec.make(*case, seed=_reference(case)[0])
    pitched = []
    for x, pad in ((obs, 3), (act, 32)):
        pitched.append(torch.zeros(b, x.shape[1] + pad, device=dev)[:, :x.shape[1]])
        pitched[-1].copy_(x.float())
    w = [p.float().contiguous().to(dev) for p in params]
    args = (pitched[0].data_ptr(), D + 3, pitched[1].data_ptr(), A + 32, b, D, A, H, E)
    return args, _C.EnsNet(*(t.data_ptr() for t in w)), [pitched, w]


def _bwd(args, net, dq, dev, want_w=True, want_a=True, short=0, fwd=True):
    """(rc, the six gradients and da [b, A] (NaN where not asked for), q) of one saving forward
    and one backward, every output and the workspace between intact guard bands."""
    b, D, A, H, E = args[4:9]
    lib = _C.lib()
    nb = int(lib.tsrl_ens_workspace_bytes(b, H, E, A))
    shapes = [(E, D + A, H), (E, 1, H), (E, H, H), (E, 1, H), (E, H, 1), (E, 1, 1), (b, A + 5)]
    bufs = [_guarded(s, dev) for s in shapes + [(E, b), (max(nb // 4, 1),)]]
    (g, da, q, ws) = [v for _, v in bufs[:6]], bufs[6][1], bufs[7][1], bufs[8][1]
    rc = lib.tsrl_ens_critic_fwd_save(*args, ctypes.byref(net), q.data_ptr(), ws.data_ptr(),
                                      nb - short, None) if fwd else 0
    if rc == 0:
        rc = lib.tsrl_ens_critic_bwd(
            *args, ctypes.byref(net), dq.data_ptr(),
            ctypes.byref(_C.EnsGrads(*(t.data_ptr() for t in g))) if want_w else None,
            da.data_ptr() if want_a else None, A + 5, ws.data_ptr(), nb - short, None)
    torch.cuda.synchronize(dev)
    assert all(_intact(full) for full, _ in bufs) and bool(da[:, A:].isnan().all())
    return rc, g + [da[:, :A]], q


@pytest.mark.parametrize("case", ec.CASES, ids=str)
def test_backward_matches_f64(dev, case):
    seed, (same, smallest, err), dq, ref32, ref64 = _reference(case)
    assert same and smallest > 16 * err, (seed, same, smallest, err)
    args, net, _keep = _case(case, dev)
    g = dq.float().to(dev)
    rc, got, q = _bwd(args, net, g, dev)
    _C.check(rc, "bwd")
    assert torch.equal(q, _fwd(args, net, dev))  # the saving forward's q is the forward's
    again = _bwd(args, net, g, dev)[1]
    worst = 0.0
    for name, x, y, r32, r64 in zip(NAMES, got, again, ref32, ref64):
        assert torch.equal(x, y), name  # a second call is bitwise equal
        ratio = ec.worst_ratio(x.cpu(), r32, r64)
        print(f"backward {case} seed {seed} {name}: error ratio to f32 {ratio:.3f}")
        worst = max(worst, ratio)
    assert worst <= 4.0


def test_phases_and_refusals(dev):
    case = ec.CASES[2]
    args, net, _keep = _case(case, dev)
    g = _reference(case)[2].float().to(dev)
    full = _bwd(args, net, g, dev)[1]
    rc, only_a, _ = _bwd(args, net, g, dev, want_w=False)
    assert rc == 0 and torch.equal(only_a[6], full[6])
    assert all(bool(t.isnan().all()) for t in only_a[:6])
    rc, only_w, _ = _bwd(args, net, g, dev, want_a=False)
    assert rc == 0 and bool(only_w[6].isnan().all())
    assert all(torch.equal(x, y) for x, y in zip(only_w[:6], full[:6]))
    # H, D + A = 513, E and an action gradient wider than TSRL_ENS_MAX_ACT_GRAD
    # (the saving forward takes any A the forward takes)
    for fwd in (True, False):
        wide = () if fwd else ((6, _C.ENS_MAX_ACT_GRAD + 1),)
        for i, v in ((7, 64), (5, 510), (8, 65)) + wide:
            rc, out, q = _bwd(args[:i] + (v,) + args[i + 1:], net, g, dev, fwd=fwd)
            assert rc == _C.ERR_ENS_SHAPE and all(bool(t.isnan().all()) for t in out + [q])
    for fwd, name in ((True, b"tsrl_ens_critic_fwd_save"), (False, b"tsrl_ens_critic_bwd")):
        rc, out, q = _bwd(args, net, g, dev, short=1, fwd=fwd)
        assert rc not in (0, _C.ERR_ENS_SHAPE) and name in _C.lib().tsrl_last_error()
        assert all(bool(t.isnan().all()) for t in out + [q])


def test_ensemble_critic_learn(dev):
    from tianshou_amd.utils.net import ensemble_critic
    torch.manual_seed(3)
    obs, act = torch.randn(33, ec.D, device=dev), torch.randn(33, ec.A, device=dev)
    dq = torch.randn(ec.MEMBERS, 33, 1, device=dev)
    critic = ec.make_critics(dev)
    w = [p.detach() for p in critic.parameters()]
    args = (obs.data_ptr(), ec.D, act.data_ptr(), ec.A, 33, ec.D, ec.A, ec.HIDDEN[0], ec.MEMBERS)
    want = _fwd(args, _C.EnsNet(*(t.data_ptr() for t in w)), dev)
    a = act.clone().requires_grad_()
    q = ensemble_critic(critic, obs, a, learn=True)
    assert torch.equal(q.detach(), want.unsqueeze(-1))
    q.backward(dq)
    got = [p.grad for p in critic.parameters()] + [a.grad]
    cpu = lambda t, dtype: t.detach().cpu().to(dtype)  # noqa: E731
    refs = [_grads([cpu(p, dt) for p in w], cpu(obs, dt), cpu(act, dt), cpu(dq, dt).squeeze(-1),
                   dt) for dt in (torch.float32, torch.float64)]
    worst = max(ec.worst_ratio(x.cpu(), r32, r64) for x, r32, r64 in zip(got, *refs))
    print(f"ensemble_critic(learn=True): worst error ratio to f32 {worst:.3f}")
    assert worst <= 4.0
    for learn in (True, "act"):  # towards the action alone: no parameter receives a gradient
        critic.zero_grad(set_to_none=True)
        a2 = act.clone().requires_grad_()
        torch.autograd.backward(ensemble_critic(critic, obs, a2, learn=learn), dq, inputs=[a2])
        assert torch.equal(a2.grad, a.grad) and all(p.grad is None for p in critic.parameters())
    for other, x, y in ((ec.make_critics(dev, activation=torch.nn.Tanh), obs, act),
                        (ec.make_critics(dev, hidden=(16, 16)), obs, act),
                        (ec.make_critics("cpu"), obs.cpu(), act.cpu())):
        assert torch.equal(ensemble_critic(other, x, y, learn=True), other(x, y))


@pytest.mark.parametrize("graph", (False, True), ids=("eager", "graph"))
def test_redq_learn_on_off(dev, graph):
    """tests/test_gpu_ensemble.py's on / off comparison for ``fused_ensemble_learn``: a
    critic-only update, then one that steps the actor.  Plain SGD is not captured, so the graph
    leg steps with Adam(lr 1, eps 100): eps is far above every gradient here (at most about 11),
    which keeps the step near lr / eps = 1e-2 times the gradient -- linear in it, as
    make_policy's SGD is, where Adam's own normalisation would turn the rounding of a cancelled
    gradient into a step of full size.  It runs five updates: each kind once eagerly (with the flag on
    a kind is captured only after an eager step of it), the two captures, one replay."""
    runs = {}
    for on in (True, False):
        policy, buf = ec.make_policy(dev, False)
        policy.fused_ensemble_learn, policy.graph_learn = on, graph
        if graph:
            policy.actor_optim = torch.optim.Adam(policy.actor.parameters(), lr=1.0, eps=100.0)
            policy.critics_optim = torch.optim.Adam(policy.critics.parameters(), lr=1.0, eps=100.0)
        before = torch.cat([p.detach().reshape(-1) for p in policy.parameters()]).clone()
        np.random.seed(ec.SEED)
        torch.manual_seed(ec.SEED)
        res = [policy.update(ec.BATCH, buf) for _ in range(5 if graph else 2)]
        assert not policy._graph_failed and len(policy._learn_graphs) == (2 if graph else 0)
        after = torch.cat([p.detach().reshape(-1) for p in policy.parameters()])
        runs[on] = (res, (after - before).cpu().double())
    (r1, d1), (r0, d0) = runs[True], runs[False]
    assert [sorted(r) for r in r1] == [sorted(r) for r in r0] and "loss/actor" in r1[1]
    print(f"redq learn on / off ({'graph' if graph else 'eager'}): deltas max abs "
          f"{float((d1 - d0).abs().max()):.3g} of {float(d0.abs().max()):.3g}")
    for a, c in zip(r1, r0):
        np.testing.assert_allclose([a[k] for k in sorted(a)], [c[k] for k in sorted(c)], rtol=1e-5)
    assert float(d0.abs().max()) > 0
    np.testing.assert_allclose(d1, d0, rtol=1e-4, atol=1e-6 * float(d0.abs().max()))
