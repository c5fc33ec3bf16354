"""csrc/gail.hip through the C ABI, and GAILPolicy.update with the fused discriminator on / off.

Bound (tests/test_gpu_fvp.py's): max-abs and 2-norm error against the f64 restatement
(tests/gail_common.py) at most 4 x the error of the same formulation in f32 on the CPU on
identical inputs, floor 2^-23 of the reference's norm; per parameter block for the gradients.
The 4 covers the other summation order (64-row tiles, one partial per workgroup) and 1 - h^2
formed from stored activations.  Every output sits between NaN guard bands.  Each test prints
its measured ratio (profiles/gail_gpu_tests.log)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import gail_common as gc
from tianshou_amd import _C

pytestmark = pytest.mark.gpu
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _guarded(n, dev):
    t = torch.full((n + 2 * GUARD,), float("nan"), device=dev)
    return t, t[GUARD:GUARD + n]


def _intact(t, n):
    return bool(t[:GUARD].isnan().all() and t[GUARD + n:].isnan().all())


def _rows(obs, act, dev, indexed, keep):
    """tsrl_gail_rows over obs / act: stored in permuted order at a 32-float-multiple obs pitch
    and read back through the permutation, or as they are with pitch D and NULL indices."""
    n, D = obs.shape
    if not indexed:
        o, a, i = obs.float().to(dev), act.float().to(dev), None
    else:
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(1))
        o = torch.zeros(n, (D + 31) // 32 * 32, device=dev)[:, :D]
        a = torch.zeros(n, act.shape[1], device=dev)
        o[perm], a[perm] = obs.float().to(dev), act.float().to(dev)
        i = perm.to(dev)
    keep += [o, a, i]
    ip = None if i is None else i.data_ptr()
    return _C.GailRows(o.data_ptr(), o.stride(0), ip, a.data_ptr(), a.stride(0), ip)


def _net(params, dev, keep):
    w = [p.float().contiguous().to(dev) for p in params]
    keep += w
    return _C.GailNet(*(t.data_ptr() for t in w))


@pytest.mark.parametrize("indexed", (True, False))
@pytest.mark.parametrize("n,_m,D,A", gc.CASES)
def test_reward_matches_f64(dev, n, _m, D, A, indexed):
    params, obs, act, *_ = gc.make(n, 1, D, A)
    keep = []
    rows, net = _rows(obs, act, dev, indexed, keep), _net(params, dev, keep)
    full, rew = _guarded(n, dev)
    _C.check(_C.lib().tsrl_gail_reward(ctypes.byref(rows), n, D, A, ctypes.byref(net),
                                       rew.data_ptr(), None), "reward")
    assert _intact(full, n)
    worst = gc.worst_ratio(rew.cpu(), gc.reward(params, obs, act, torch.float32),
                           gc.reward(params, obs, act))
    print(f"reward n={n} D={D} A={A} indexed={indexed}: worst error ratio to f32 {worst:.3f}")
    assert worst <= 4.0


@pytest.mark.parametrize("m_pi,m_exp,D,A", gc.CASES)
def test_step_matches_f64(dev, m_pi, m_exp, D, A):
    params, obs, act, eobs, eact, eidx = gc.make(m_pi, m_exp, D, A)
    x_pi, x_exp = torch.cat([obs, act], 1), torch.cat([eobs, eact], 1)[eidx]
    ref64 = gc.disc_step(params, x_pi, x_exp)
    ref32 = gc.disc_step(params, x_pi, x_exp, torch.float32)
    keep = []
    pi, net = _rows(obs, act, dev, True, keep), _net(params, dev, keep)
    ex = _rows(eobs, eact, dev, False, keep)
    keep.append(eidx.to(dev))
    ex.io = ex.ia = keep[-1].data_ptr()  # draws with replacement: rows repeat
    P = sum(p.numel() for p in params)
    nb = int(_C.lib().tsrl_gail_disc_step_workspace_bytes(m_pi, m_exp, D, A))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    outs = []
    for _ in range(2):
        (gfull, grad), (ofull, out3) = _guarded(P, dev), _guarded(3, dev)
        _C.check(_C.lib().tsrl_gail_disc_step(
            ctypes.byref(pi), m_pi, ctypes.byref(ex), m_exp, D, A, ctypes.byref(net),
            grad.data_ptr(), out3.data_ptr(), ws.data_ptr(), nb, None), "step")
        assert _intact(gfull, P) and _intact(ofull, 3)
        outs.append((grad.cpu(), out3.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    grad, out3 = outs[0]
    assert float(out3[1]) == float(ref64[1].float()) and float(out3[2]) == float(ref64[2].float())
    worst = max(gc.worst_ratio(grad, ref32[3], ref64[3], params),
                gc.worst_ratio(out3[:1], ref32[0], ref64[0]))
    print(f"step m_pi={m_pi} m_exp={m_exp} D={D} A={A}: worst error ratio to f32 {worst:.3f}")
    assert worst <= 4.0


def test_argument_errors(dev):
    params, obs, act, *_ = gc.make(4, 1, 3, 1)
    keep = []
    rows, net = _rows(obs, act, dev, False, keep), _net(params, dev, keep)
    full, rew = _guarded(4, dev)
    L = _C.lib()
    assert L.tsrl_gail_reward(ctypes.byref(rows), 0, 3, 1, ctypes.byref(net), None, None) == 0
    rows.ldo = 2  # shorter than D
    assert L.tsrl_gail_reward(ctypes.byref(rows), 4, 3, 1, ctypes.byref(net), rew.data_ptr(),
                              None) != 0 and b"pitch" in L.tsrl_last_error()
    rows.ldo = 3
    assert L.tsrl_gail_disc_step(ctypes.byref(rows), 0, ctypes.byref(rows), 4, 3, 1,
                                 ctypes.byref(net), rew.data_ptr(), rew.data_ptr(),
                                 rew.data_ptr(), 16, None) != 0
    assert L.tsrl_gail_disc_step(ctypes.byref(rows), 4, ctypes.byref(rows), 4, 3, 1,
                                 ctypes.byref(net), rew.data_ptr(), rew.data_ptr(),
                                 rew.data_ptr(), 16, None) != 0 and \
        b"workspace" in L.tsrl_last_error()
    torch.cuda.synchronize()
    assert bool(full.isnan().all())  # nothing was launched


@pytest.mark.parametrize("num", (4, 3))  # 320 rows: four even splits; 106, 106 and a merged 108
def test_update_fused_matches_unfused(dev, num, monkeypatch):
    n, runs, calls, L = gc.E * gc.T, {}, [], _C.lib()
    monkeypatch.setattr(L, "tsrl_gail_disc_step", (lambda f: lambda *a: (
        calls.append(1), f(*a))[1])(L.tsrl_gail_disc_step))
    for fused in (True, False):
        policy, buf = gc.make_policy(dev, fused, num)
        init = [p.detach().cpu().clone() for p in policy.disc_net.parameters()]
        batch = buf.sample(0)[0]
        rew = policy.disc_reward(batch).cpu()
        obs, act = batch.obs.cpu(), batch.act.cpu()
        np.random.seed(7)
        calls.clear()
        res = policy.update(0, buf, batch_size=80, repeat=2)
        assert len(calls) == (num if fused else 0)
        runs[fused] = (res, rew, torch.cat([p.detach().cpu().reshape(-1)
                                            for p in policy.disc_net.parameters()]),
                       np.random.get_state()[1].copy(), np.random.get_state()[2])
    assert policy._disc is not None and runs[True][0].keys() == runs[False][0].keys()
    np.random.seed(7)
    first = []
    *lists64, p64 = gc.disc_phase_f64(init, obs, act, gc.policy_data()[1], n, num,
                                      first_grad=first)
    (rf, rewf, pf, *sf), (rt, rewt, pt, *st) = runs[True], runs[False]
    assert np.array_equal(sf[0], st[0]) and sf[1] == st[1]  # np.random left in the same state
    worst = gc.worst_ratio(rewf, rewt, gc.reward(init, obs, act))
    for k, ref in zip(("loss/disc", "stats/acc_pi", "stats/acc_exp"), lists64):
        assert len(rf[k]) == len(rt[k]) == len(ref) and len(rf["loss"]) == len(rt["loss"])
        worst = max(worst, gc.worst_ratio(rf[k], rt[k], ref))
    # Adam's first step is sign-like: elements whose first gradient is tiny are left out
    keep = torch.cat([g.abs() >= 1e-6 * g.abs().max() for g in gc.split(first[0], init)])
    assert float((~keep).double().mean()) <= 0.01
    flat64 = torch.cat([t.reshape(-1) for t in p64])
    worst = max(worst, gc.worst_ratio(pf[keep], pt[keep], flat64[keep]))
    print(f"update disc_update_num={num}: worst error ratio of the fused leg to the torch leg "
         f"{worst:.3f}")
    assert worst <= 4.0
