"""BranchingDQNPolicy on the device path (tianshou_amd/policy/bdq.py, utils/net.py BranchingNet,
env/wrappers.py ContinuousToDiscrete, csrc/bdq.hip) against f64 NumPy restatements (kernels)
and against the reference run recorded in tests/golden/bdq.npz (tools/gen_goldens.py gen_bdq;
tests/test_bdq_host.py pins that file and holds the restatements).

Kernel shapes are the lane, wave, workgroup and multi-partial edges (b 1 .. 1000, K 1 .. 17,
A 1 .. 65), not workload sizes.  Tolerances: combine forward 1 ulp32 of the rounded f64 value
and the argmax of the written tensor exact; combine backward rtol 1e-5 / atol 1e-6 * max|ref|;
target rtol 1e-6; loss rtol 1e-5, grad_q and prio rtol 1e-4 / atol 1e-6 * max|ref|.  update()
against the recording: sampled indices equal, returns rtol 1e-5 / atol 1e-6, losses rtol 2e-5 /
atol 1e-6, outgoing weights rtol 1e-4 (every recorded |sum_k td| >= 1e-2), Adam parameters,
online and target, rtol 1e-5 / atol 1e-6, prioritized leaves and priorities rtol 1e-4 (DESIGN.md
section 4).  With RMSprop the parameter bound is 4 x what the torch formulation of the same
policy (``fused = False``) deviates from the same recording on the same GPU (TORCH_DEV)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import test_bdq_host as bh
from tianshou_amd import _C
from tianshou_amd.policy import BranchingDQNPolicy
from tianshou_amd.policy import dqn as dqn_mod
from tianshou_amd.policy.bdq import _BDQLoss, bdq_target_device

pytestmark = pytest.mark.gpu

for _name in bh.SYMBOLS:
    assert _name in _C.EXPORTED

# max |parameter - recorded| of the torch formulation (fused = False) after each of the six
# updates of the "rms" variant, measured on an MI355X against tests/golden/bdq.npz.  An early
# RMSprop step is lr * g / (0.1 |g| + eps): where |g| ~ eps it moves with the last bits of g.
TORCH_DEV = {
    "rms": (2.98e-8, 2.98e-8, 2.98e-8, 3.73e-8, 3.73e-8, 3.73e-8),
}
# The fused path measured 2.98e-8, 5.96e-8, 5.96e-8, 5.96e-8, 5.96e-8, 5.96e-8 in the same
# session, eager and graph-replayed alike (one ulp of the largest parameters).

BS = (1, 63, 64, 65, 257, 1000)
KS = (1, 2, 4, 17)
AS = (1, 2, 25, 64, 65)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "bdq.npz"))


@pytest.fixture(scope="module")
def cfg(z):
    return json.loads(str(z["learn_cfg"]))


def _d(t, dev):
    return None if t is None else torch.as_tensor(t).to(dev).contiguous()


# -- combine ----------------------------------------------------------------------------------------
def _combine_fwd(s, v, want_act=True):
    b, K, A = s.shape
    out = torch.full_like(s, float("nan"))
    act = torch.full((b, K), -7, dtype=torch.int64, device=s.device) if want_act else None
    _C.check(_C.lib().tsrl_bdq_combine_fwd(_C.ptr(s), _C.ptr(v), b, K, A, _C.ptr(out),
                                           _C.ptr(act), _C.stream_ptr(s.device)), "combine_fwd")
    return out, act


def _combine_cases(b, K, A, g):
    yield "random", torch.randn(b, K, A, generator=g), torch.randn(b, generator=g)
    # few distinct values: most branches hold their maximum more than once
    yield "ties", torch.randint(-2, 2, (b, K, A), generator=g).float() / 2, \
        torch.randn(b, generator=g)
    yield "constant", torch.full((b, K, A), 0.25), torch.randn(b, generator=g)
    s = torch.randn(b, K, A, generator=g)
    s[b // 2, K // 2, A // 2] = float("nan")
    yield "nan", s, torch.randn(b, generator=g)


@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("b", BS)
def test_combine_fwd_matches_f64(dev, b, A):
    for K in KS:
        g = torch.Generator().manual_seed(10000 * b + 100 * K + A)
        for name, s, v in _combine_cases(b, K, A, g):
            s64, v64 = s.double().numpy(), v.double().numpy()
            with np.errstate(invalid="ignore"):
                want = (v64[:, None, None] + (s64 - s64.mean(2, keepdims=True))) \
                    .astype(np.float32)
            out, act = _combine_fwd(_d(s, dev), _d(v, dev))
            got = out.cpu().numpy()
            tag = f"{name} b {b} K {K} A {A}"
            assert np.array_equal(np.isnan(got), np.isnan(want)), tag
            ok = ~np.isnan(want)
            if name == "nan":
                assert np.isnan(got[b // 2, K // 2]).all() and np.isnan(got).sum() == A, tag
            # the f64 mean may be summed in another order: 1 ulp32 of the rounded f64 value
            assert (np.abs(got[ok] - want[ok]) <= np.spacing(np.abs(want[ok]))).all(), tag
            if (A == 1 and name != "nan") or name == "constant":
                assert np.array_equal(got, np.broadcast_to(v.numpy()[:, None, None], got.shape))
            # NumPy's argmax: the first index of the maximum, the first NaN if there is one
            assert np.array_equal(act.cpu().numpy(), got.argmax(axis=2)), tag
            if name == "random":  # no ties: torch's own max on the written tensor
                assert torch.equal(act, out.max(-1)[1]), tag
            out2, none = _combine_fwd(_d(s, dev), _d(v, dev), want_act=False)
            assert none is None and np.array_equal(out2.cpu().numpy(), got, equal_nan=True), tag


def test_combine_fwd_argmax_takes_the_first_nan_and_the_first_maximum(dev):
    s = torch.zeros(3, 2, 70)
    s[0, 0, 66], s[0, 0, 3] = 5.0, 5.0          # a tie across the 64-lane stride: index 3
    s[0, 1, 69] = 1.0                            # the maximum in the second pass of the lanes
    s[1, 0, 65], s[1, 0, 2] = float("inf"), float("nan")
    s[2, 1, 0] = -1.0                            # every other entry ties at the maximum: 1
    out, act = _combine_fwd(_d(s, dev), torch.zeros(3, device=dev))
    assert act.tolist() == [[3, 69], [0, 0], [0, 1]]  # NaN mean: a whole NaN branch, index 0
    assert np.array_equal(act.cpu().numpy(), out.cpu().numpy().argmax(2))


def _combine_bwd(g):
    b, K, A = g.shape
    g_s = torch.full_like(g, float("nan"))
    g_v = torch.full((b,), float("nan"), device=g.device)
    _C.check(_C.lib().tsrl_bdq_combine_bwd(_C.ptr(g), b, K, A, _C.ptr(g_s), _C.ptr(g_v),
                                           _C.stream_ptr(g.device)), "combine_bwd")
    return g_s, g_v


@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("b", BS)
def test_combine_bwd_matches_f64_and_autograd(dev, b, A):
    for K in KS:
        gen = torch.Generator().manual_seed(20000 * b + 100 * K + A)
        g = torch.randn(b, K, A, generator=gen)
        g64 = g.double().numpy()
        want_s, want_v = g64 - g64.mean(2, keepdims=True), g64.sum((1, 2))
        gd = _d(g, dev)
        g_s, g_v = _combine_bwd(gd)
        tag = f"b {b} K {K} A {A}"
        np.testing.assert_allclose(g_s.cpu().numpy(), want_s, rtol=1e-5,
                                   atol=1e-6 * np.abs(want_s).max() + 1e-30, err_msg=tag)
        np.testing.assert_allclose(g_v.cpu().numpy(), want_v, rtol=1e-5,
                                   atol=1e-6 * np.abs(want_v).max(), err_msg=tag)
        # torch autograd through the torch lines (common.py:537-543), f32 on the device
        s = torch.randn(b, K, A, generator=gen).to(dev).requires_grad_(True)
        v = torch.randn(b, 1, generator=gen).to(dev).requires_grad_(True)
        logits = torch.unsqueeze(v, 1) + (s - torch.mean(s, 2, keepdim=True))
        logits.backward(gd)
        torch.testing.assert_close(g_s, s.grad, rtol=1e-5, atol=1e-6 * float(np.abs(want_s).max()))
        torch.testing.assert_close(g_v, v.grad[:, 0], rtol=1e-5,
                                   atol=1e-6 * float(np.abs(want_v).max()))
        again = _combine_bwd(gd)  # a fixed summation order: the same bits every launch
        assert torch.equal(again[0], g_s) and torch.equal(again[1], g_v), tag


def test_branching_net_routes_through_the_combine_kernels(dev, monkeypatch):
    from tianshou_amd.utils.net import BranchingNet
    torch.manual_seed(3)
    net = BranchingNet(7, 3, 5, [16], [8], [8], device=dev).to(dev)
    obs = torch.randn(33, 7, device=dev)
    calls = _count_calls(monkeypatch)
    with torch.no_grad():
        logits, _ = net(obs)
    assert calls == {"tsrl_bdq_combine_fwd": 1}
    act = net.greedy_act(logits)
    assert act is not None and torch.equal(act, logits.max(-1)[1])
    assert net.greedy_act(logits.clone()) is None
    logits_g, _ = net(obs)  # with gradients: no act, and a kernel backward
    assert net.greedy_act(logits_g) is None and torch.equal(logits_g, logits)
    g = torch.randn_like(logits_g)
    logits_g.backward(g)
    assert calls == {"tsrl_bdq_combine_fwd": 2, "tsrl_bdq_combine_bwd": 1}
    grads = [p.grad.clone() for p in net.parameters()]
    net.zero_grad()
    net.fused_combine = False
    logits_t, _ = net(obs)
    logits_t.backward(g)
    assert calls == {"tsrl_bdq_combine_fwd": 2, "tsrl_bdq_combine_bwd": 1}
    torch.testing.assert_close(logits_t, logits, rtol=1e-5, atol=1e-6)
    for a, p in zip(grads, net.parameters()):
        torch.testing.assert_close(a, p.grad, rtol=1e-4, atol=1e-5 * float(a.abs().max()))
    net.fused_combine = True
    assert net(obs.double().cpu().numpy())[0].dtype == torch.float32  # MLP casts to f32
    assert net(obs[:0])[0].shape == (0, 3, 5)  # b == 0: the torch lines, nothing launched
    assert calls["tsrl_bdq_combine_fwd"] == 3


class _CountingLib:
    def __init__(self, real, calls):
        self._real, self._calls = real, calls

    def __getattr__(self, name):
        if name.startswith("tsrl_bdq_"):
            self._calls[name] = self._calls.get(name, 0) + 1
        return getattr(self._real, name)


def _count_calls(monkeypatch):
    """Calls of the tsrl_bdq_* entry points from here on, by name."""
    calls = {}
    monkeypatch.setattr(_C, "_LIB", _CountingLib(_C.lib(), calls))
    return calls


# -- target -----------------------------------------------------------------------------------------
def _target_ref(q_sel, q_eval, rew, end, gamma):
    arg = q_sel.argmax(axis=2)  # NumPy: the first maximum, the first NaN
    m = np.take_along_axis(q_eval.astype(np.float64), arg[..., None], 2)[..., 0].mean(1)
    with np.errstate(invalid="ignore"):
        return rew + gamma * m * (1.0 - end)


def _rows_gap(q):
    q = np.sort(q.astype(np.float64), axis=-1)
    return (q[..., -1] - q[..., -2]) / np.maximum(np.abs(q[..., -1]), np.abs(q[..., -2]))


@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("b", BS)
def test_target_matches_f64(dev, b, A):
    gamma = 0.97
    for K in KS:
        g = torch.Generator().manual_seed(30000 * b + 100 * K + A)
        rew = torch.randn(b, generator=g, dtype=torch.float64)
        end = torch.rand(b, generator=g) < 0.3
        if b > 1:
            end[0], end[1] = True, False
        cases = {
            "random": (torch.randn(b, K, A, generator=g), torch.randn(b, K, A, generator=g)),
            "ties": (torch.randint(-2, 2, (b, K, A), generator=g).float() / 2,
                     torch.randn(b, K, A, generator=g)),
            "constant": (torch.full((b, K, A), 0.25), torch.randn(b, K, A, generator=g)),
        }
        s_nan = torch.randn(b, K, A, generator=g)
        s_nan[:, K // 2, A - 1] = float("nan")  # the NaN wins its branch in every row
        cases["nan_sel"] = (s_nan, torch.randn(b, K, A, generator=g))
        for name, (q_sel, q_eval) in cases.items():
            tag = f"{name} b {b} K {K} A {A}"
            qs, qe = q_sel.numpy(), q_eval.numpy()
            if name == "random" and A > 1:  # no row is excluded from the index comparison
                assert _rows_gap(qs).min() >= 1e-6 and _rows_gap(qe).min() >= 1e-6, tag
            e = end.numpy().astype(np.float64)
            got = bdq_target_device(_d(q_sel, dev), _d(q_eval, dev), _d(rew, dev), _d(end, dev),
                                    gamma, True).cpu().numpy()
            assert got.dtype == np.float32
            np.testing.assert_allclose(got, _target_ref(qs, qe, rew.numpy(), e, gamma),
                                       rtol=1e-6, err_msg=tag)
            # an ended row is exactly the rounded reward
            assert np.array_equal(got[end.numpy()], rew.numpy().astype(np.float32)[end.numpy()])
            if name == "nan_sel":
                continue
            # Nature DQN: the argmax of q_eval itself, q_sel unread (NULL)
            nat = bdq_target_device(None, _d(q_eval, dev), _d(rew, dev), _d(end, dev), gamma,
                                    False).cpu().numpy()
            np.testing.assert_allclose(nat, _target_ref(qe, qe, rew.numpy(), e, gamma),
                                       rtol=1e-6, err_msg=tag)
            # no target network: both arguments are the same tensor
            same = _d(q_sel, dev)
            one = bdq_target_device(same, same, _d(rew, dev), _d(end, dev), gamma, True)
            np.testing.assert_allclose(one.cpu().numpy(),
                                       _target_ref(qs, qs, rew.numpy(), e, gamma), rtol=1e-6)
            two = bdq_target_device(None, same, _d(rew, dev), _d(end, dev), gamma, False)
            assert torch.equal(one, two), tag


def test_target_selects_by_index_and_keeps_nan_on_ended_rows(dev):
    """K 1, gamma 1, reward 0: the output is the selected q_eval entry itself, so the selected
    index is read off exactly -- the first maximum, a NaN ahead of every number."""
    A = 70
    q_sel = torch.zeros(4, 1, A)
    q_sel[0, 0, 66], q_sel[0, 0, 5] = 2.0, 2.0
    q_sel[1, 0, 68], q_sel[1, 0, 9] = float("nan"), float("inf")
    q_sel[2, 0, 69] = 1.0
    q_eval = torch.arange(4 * A, dtype=torch.float32).reshape(4, 1, A)
    zero, live = torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.bool)
    got = bdq_target_device(_d(q_sel, dev), _d(q_eval, dev), _d(zero, dev), _d(live, dev), 1.0,
                            True)
    assert got.tolist() == [5.0, A + 68.0, 2 * A + 69.0, 3.0 * A]
    # NaN * 0 stays NaN: an ended row whose selected value is NaN
    q_eval[3, 0, 0] = float("nan")
    got = bdq_target_device(_d(q_sel, dev), _d(q_eval, dev), _d(zero + 1.5, dev),
                            _d(~live, dev), 1.0, True)
    assert got[:3].tolist() == [1.5, 1.5, 1.5] and bool(got[3].isnan())


# -- loss -------------------------------------------------------------------------------------------
def _td_inputs(b, K, A, weighted, dev, seed=0):
    g = torch.Generator().manual_seed(77 * b + 1000 * K + A + seed)
    q = torch.randn(b, K, A, generator=g)
    act = torch.randint(0, A, (b, K), generator=g)
    returns = torch.randn(b, generator=g) * 2
    weight = torch.rand(b, generator=g) + 0.1 if weighted else None
    return tuple(_d(t, dev) for t in (q, act, returns, weight))


def _bdq_loss(q, act, returns, weight):
    q_k = q.clone().requires_grad_(True)
    loss, prio = _BDQLoss.apply(q_k, (act, returns, weight, None, None))
    loss.backward()
    return loss.detach().clone(), prio.clone(), q_k.grad.clone()


def _check_td(q, act, returns, weight, tag):
    loss, prio, grad = _bdq_loss(q, act, returns, weight)
    np_ = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    want_loss, want_prio, want_grad = bh.td_reference(np_(q), np_(act), np_(returns),
                                                      np_(weight))
    np.testing.assert_allclose(loss.item(), want_loss, rtol=1e-5, err_msg=tag)
    np.testing.assert_allclose(np_(prio), want_prio, rtol=1e-4,
                               atol=1e-6 * np.abs(want_prio).max(), err_msg=tag)
    np.testing.assert_allclose(np_(grad), want_grad, rtol=1e-4,
                               atol=1e-6 * np.abs(want_grad).max(), err_msg=tag)
    off = torch.ones_like(grad, dtype=torch.bool)
    off.scatter_(2, act.unsqueeze(-1), False)
    g_off = grad[off]
    assert (g_off == 0).all() and not torch.signbit(g_off).any(), tag  # exactly +0
    again = _bdq_loss(q, act, returns, weight)  # a fixed summation order: the same bits
    assert all(torch.equal(a, c) for a, c in zip((loss, prio, grad), again)), tag
    return loss, prio, grad


@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("b", BS)
def test_td_fwd_bwd_matches_f64(dev, b, A, weighted):
    for K in KS:
        q, act, returns, weight = _td_inputs(b, K, A, weighted, dev)
        _check_td(q, act, returns, weight, f"b {b} K {K} A {A} weighted {weighted}")


@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("b", BS)
def test_td_one_branch_is_the_dqn_kernel_bit_for_bit(dev, b, A, weighted):
    from tianshou_amd.policy.dqn import _DQNLoss
    q, act, returns, weight = _td_inputs(b, 1, A, weighted, dev, seed=5)
    loss, prio, grad = _bdq_loss(q, act, returns, weight)
    q_k = q.reshape(b, A).clone().requires_grad_(True)
    loss_d, td_d = _DQNLoss.apply(q_k, (act.reshape(b), returns, weight, False, None, None))
    loss_d.backward()
    assert torch.equal(loss, loss_d.detach()) and torch.equal(prio, td_d)
    assert torch.equal(grad.reshape(b, A), q_k.grad)
    assert torch.equal(torch.signbit(grad.reshape(b, A)), torch.signbit(q_k.grad))


@pytest.mark.parametrize("b", (65, 257))  # one workgroup, and partials with the fold
def test_td_constructed_rows(dev, b):
    K, A = 4, 25
    q, act, returns, weight = _td_inputs(b, K, A, True, dev, seed=9)
    rows = torch.arange(b, device=dev)
    # row 3: td = 0 in every branch (all taken Q-values equal the return exactly)
    q[3].scatter_(1, act[3].unsqueeze(-1), returns[3].expand(K, 1).clone())
    weight[5] = 0.0                      # row 5: zero weight
    returns[7] = 3e18                    # row 7: |td| = 3e18, td^2 = 9e36 still an f32
    loss, prio, grad = _check_td(q, act, returns, weight, f"constructed b {b}")
    assert prio[3] == 0 and (grad[3] == 0).all() and (grad[5] == 0).all()
    assert float(prio[7]) == pytest.approx(K * 3e18, rel=1e-6) and bool(torch.isfinite(loss))
    # one invalid action in one branch of one row: that row alone is lost
    for bad in (A, -1):
        act_bad = act.clone()
        act_bad[b - 2, K - 1] = bad
        loss_b, prio_b, grad_b = _bdq_loss(q, act_bad, returns, weight)
        assert bool(loss_b.isnan()) and bool(prio_b[b - 2].isnan())
        assert (grad_b[b - 2] == 0).all() and not torch.signbit(grad_b[b - 2]).any()
        keep = rows != b - 2
        assert torch.equal(prio_b[keep], prio[keep]) and torch.equal(grad_b[keep], grad[keep])


def test_bdq_loss_seed_paths_and_static_outputs(dev):
    from tianshou_amd.policy.onpolicy import _unit_seed
    q, act, returns, weight = _td_inputs(257, 4, 25, True, dev)
    grads = []
    for seed in ("ones", "unit", 2.5):
        q_k = q.clone().requires_grad_(True)
        loss, _ = _BDQLoss.apply(q_k, (act, returns, weight, None, None))
        if seed == "ones":
            loss.backward()
        elif seed == "unit":
            loss.backward(_unit_seed(dev))
        else:
            (loss * seed).backward()
        grads.append(q_k.grad.clone())
    assert torch.equal(grads[0], grads[1])
    torch.testing.assert_close(grads[2], 2.5 * grads[0], rtol=1e-6, atol=0)
    td_out = torch.zeros(257, device=dev)
    loss_out = torch.zeros((), device=dev)
    loss2, td2 = _BDQLoss.apply(q.clone().requires_grad_(True),
                                (act, returns, weight, td_out, loss_out))
    assert td2.data_ptr() == td_out.data_ptr() and torch.equal(loss2, loss_out) and torch.equal(loss2, loss.detach())


# -- exploration_noise ------------------------------------------------------------------------------
def test_exploration_noise_on_device_act_is_the_recordings(z, dev):
    from tianshou_amd.data import Batch
    from tianshou_amd.utils.net import BranchingNet
    cases = json.loads(str(z["noise_cfg"]))
    for i, c in enumerate(cases):
        p = f"noise{i}_"
        policy = BranchingDQNPolicy(BranchingNet(3, c["K"], c["A"], [4], [4], [4]), None)
        policy.set_eps(c["eps"])
        act = torch.as_tensor(z[p + "act_in"], device=dev)
        batch = Batch(obs=torch.zeros(c["bsz"], 3, device=dev))
        np.random.seed(c["seed"])
        out = policy.exploration_noise(act, batch)
        assert out is act and out.is_cuda and out.dtype == torch.int64
        np.testing.assert_array_equal(out.cpu().numpy(), z[p + "act_out"], err_msg=p)
        st = np.random.get_state()
        np.testing.assert_array_equal(st[1], z[p + "state_keys"], err_msg=p)
        assert st[2] == int(z[p + "state_pos"]), p
    policy.set_eps(0.0)
    before = np.random.get_state()
    act_in = torch.as_tensor(z[p + "act_in"], device=dev)
    assert torch.equal(policy.exploration_noise(act_in.clone(), batch), act_in)
    after = np.random.get_state()
    assert np.array_equal(before[1], after[1]) and before[2] == after[2]


# -- update() against the recording -----------------------------------------------------------------
def _filled_buffer(z, cfg, tag, dev):
    from tianshou_amd.data import Batch, PrioritizedVectorReplayBuffer, VectorReplayBuffer
    E, S = cfg["E"], cfg["S"]
    buf = PrioritizedVectorReplayBuffer(E * S, E, alpha=0.6, beta=0.4, device=dev) \
        if cfg["variants"][tag].get("per") else VectorReplayBuffer(E * S, E, device=dev)
    o = 0
    for k in z["add_len"]:
        sl = slice(o, o + int(k))
        row = {key: z["add_" + key][sl] for key in ("obs", "rew", "terminated", "truncated",
                                                    "obs_next")}
        buf.add(Batch(act=z[tag + "_add_act"][sl], **row), buffer_ids=z["add_ids"][sl])
        o += int(k)
    return buf


def _record(policy):
    process_fn, learn, seen = policy.process_fn, policy.learn, []

    def rec_process(batch, buffer, indices):
        batch = process_fn(batch, buffer, indices)
        seen.append(dict(indices=np.array(indices, copy=True), returns=batch.returns))
        if "weight" in batch:
            seen[-1]["weight"] = batch.weight.clone()
        return batch

    def rec_learn(batch, **kw):
        res = learn(batch, **kw)
        seen[-1]["td_error"] = batch.weight.clone()
        return res

    policy.process_fn, policy.learn = rec_process, rec_learn
    return seen


def _run_variant(z, cfg, dev, tag, check_params, **attrs):
    """Six update() calls of one recorded variant; everything but the parameters is asserted
    here, the parameters by ``check_params(u, policy)``."""
    policy, v = bh.make_policy(z, cfg, tag, dev, **attrs)
    buf = _filled_buffer(z, cfg, tag, dev)
    seen = _record(policy)
    np.random.seed(cfg["checks"][tag]["seed"])
    K, A, p = v["K"], v["A"], tag + "_"
    for u in range(cfg["updates"]):
        res = policy.update(v["bs"], buf)
        s = seen[u]
        assert s["indices"].tolist() == z[p + "indices"][u].tolist(), (tag, u)
        ret = s["returns"]
        assert ret.shape == (v["bs"], K, A) and ret.is_cuda
        assert ret.untyped_storage().nbytes() == 4 * v["bs"]  # a zero-copy expand of [b]
        assert ret.dtype == torch.float32
        np.testing.assert_allclose(ret[:, 0, 0].cpu().numpy(), z[p + "returns"][u], rtol=1e-5,
                                   atol=1e-6, err_msg=f"{tag} {u}")
        np.testing.assert_allclose(res["loss"], float(z[p + "loss"][u]), rtol=2e-5, atol=1e-6,
                                   err_msg=f"{tag} {u}")
        td = s["td_error"]
        assert td.is_cuda and not td.requires_grad and td.shape == (v["bs"],)
        np.testing.assert_allclose(td.cpu().numpy(), z[p + "td_error"][u], rtol=1e-4,
                                   err_msg=f"{tag} {u}")
        if v.get("per"):
            assert s["weight"].dtype == torch.float32
            # the importance weights come from leaves held to rtol 1e-4
            np.testing.assert_allclose(s["weight"].cpu().numpy(), z[p + "weight"][u], rtol=1e-4)
            leaves = buf.weight[np.arange(buf.maxsize)]
            np.testing.assert_allclose(np.asarray(leaves), z[p + "leaves"][u], rtol=1e-4)
        check_params(u, policy)
    if v.get("per"):
        np.testing.assert_allclose(buf._max_prio, float(z[p + "max_prio"]), rtol=1e-4)
        np.testing.assert_allclose(buf._min_prio, float(z[p + "min_prio"]), rtol=1e-4)
    assert policy._iter == cfg["updates"]
    return policy


def _adam_check(z, cfg, tag):
    def check(u, policy):
        np.testing.assert_allclose(bh.flat(policy.model), z[tag + "_params"][u], rtol=1e-5,
                                   atol=1e-6, err_msg=f"{tag} update {u}")
        if cfg["variants"][tag]["freq"] > 0:  # the recorded sync points
            np.testing.assert_allclose(bh.flat(policy.model_old), z[tag + "_params_old"][u],
                                       rtol=1e-5, atol=1e-6, err_msg=f"{tag} target {u}")
    return check


LEGS = {"graph": dict(graph_learn=True), "eager": dict(graph_learn=False),
        "torch": dict(fused=False)}
ADAM_TAGS = ("double_target", "nature", "notarget", "per", "one_branch")


@pytest.mark.parametrize("leg", tuple(LEGS))
@pytest.mark.parametrize("tag", ADAM_TAGS)
def test_update_matches_reference_adam(z, cfg, dev, tag, leg, monkeypatch):
    calls = _count_calls(monkeypatch)
    policy = _run_variant(z, cfg, dev, tag, _adam_check(z, cfg, tag), **LEGS[leg])
    v, n = cfg["variants"][tag], cfg["updates"]
    if leg == "torch":
        # fused = False: the combine kernel inside the network still runs, nothing else
        assert policy._flat is None and not policy._learn_graphs
        assert set(calls) <= {"tsrl_bdq_combine_fwd", "tsrl_bdq_combine_bwd"}
        return
    assert policy._flat is not None and policy._flat.adam_bound(policy.optim)
    assert len(policy._learn_graphs) == (1 if leg == "graph" else 0) and not policy._graph_failed
    assert calls["tsrl_bdq_target"] == n
    # the first update runs eagerly, every later one replays a graph captured once
    assert calls["tsrl_bdq_td_fwd_bwd"] == (2 if leg == "graph" else n)
    if v["freq"] > 0:
        assert policy._old_flat is not None


def test_update_matches_reference_rmsprop(z, cfg, dev):
    """Measured on an MI355X, max |parameter - recorded| after each update: see TORCH_DEV and
    the figures this test prints (the torch leg is measured again here, the bound is the
    recorded constant)."""
    devs = {}

    def measure(leg):
        devs[leg] = []
        return lambda u, policy: devs[leg].append(float(np.abs(
            bh.flat(policy.model).astype(np.float64) - z["rms_params"][u]).max()))

    for leg in ("torch", "eager", "graph"):
        policy = _run_variant(z, cfg, dev, "rms", measure(leg), **LEGS[leg])
        print(f"rms {leg}: max|dparam| per update", " ".join(f"{d:.3g}" for d in devs[leg]))
    assert policy._flat.adam_bound(policy.optim)
    assert set(policy.optim.state[next(policy.model.parameters())]) == {"step", "square_avg"}
    for leg in ("eager", "graph"):
        for u, d in enumerate(devs[leg]):
            assert d <= 4 * TORCH_DEV["rms"][u], (leg, u, d)


# -- paths taken ------------------------------------------------------------------------------------
def _updates(z, cfg, dev, tag, sizes, **attrs):
    policy, v = bh.make_policy(z, cfg, tag, dev, **attrs)
    buf = _filled_buffer(z, cfg, tag, dev)
    np.random.seed(cfg["checks"][tag]["seed"])
    losses = [policy.update(bs, buf)["loss"] for bs in sizes]
    return policy, losses, [p.detach().clone() for p in policy.model.parameters()], buf


@pytest.mark.parametrize("tag", ("double_target", "nature", "per", "one_branch"))
def test_graph_replay_is_bitwise_eager(z, cfg, dev, tag):
    bs = cfg["variants"][tag]["bs"]
    pol_g, loss_g, par_g, buf_g = _updates(z, cfg, dev, tag, [bs] * 6, graph_learn=True)
    pol_e, loss_e, par_e, buf_e = _updates(z, cfg, dev, tag, [bs] * 6, graph_learn=False)
    assert len(pol_g._learn_graphs) == 1 and not pol_e._learn_graphs
    assert loss_g == loss_e
    for a, b in zip(par_g, par_e):
        assert torch.equal(a, b)
    if tag == "per":
        rows = np.arange(buf_g.maxsize)
        assert np.array_equal(np.asarray(buf_g.weight[rows]), np.asarray(buf_e.weight[rows]))


def test_graph_replay_follows_batch_size(z, cfg, dev):
    sizes = [64, 64, 32, 64, 32, 32]
    pol_g, loss_g, par_g, _ = _updates(z, cfg, dev, "double_target", sizes, graph_learn=True)
    pol_e, loss_e, par_e, _ = _updates(z, cfg, dev, "double_target", sizes, graph_learn=False)
    assert sorted(k[0] for k in pol_g._learn_graphs) == [32, 64]
    assert loss_g == loss_e
    for a, b in zip(par_g, par_e):
        assert torch.equal(a, b)


def test_default_replays_two_dimensional_observations(z, cfg, dev):
    policy, _, _, _ = _updates(z, cfg, dev, "double_target", [32] * 3)
    assert policy.graph_learn is None and len(policy._learn_graphs) == 1


def test_graphs_are_dropped_when_flat_storage_moves(z, cfg, dev):
    policy, _, _, buf = _updates(z, cfg, dev, "double_target", [32, 32, 64, 64],
                                 graph_learn=True)
    assert len(policy._learn_graphs) == 2
    flat = policy._flat.flat_param
    policy.optim = torch.optim.Adam(policy.model.parameters(), lr=1e-3)
    losses = [policy.update(32, buf)["loss"] for _ in range(2)]
    assert policy._flat.flat_param.data_ptr() != flat.data_ptr()
    assert len(policy._learn_graphs) == 1 and next(iter(policy._learn_graphs))[0] == 32
    assert all(np.isfinite(losses))


def test_capture_failure_warns_once_and_stays_eager(z, cfg, dev, monkeypatch):
    import warnings
    tries = []

    def failing_capture(graph):
        tries.append(graph)
        raise RuntimeError("simulated capture failure")

    monkeypatch.setattr(dqn_mod, "graph_capture", failing_capture)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        policy = _run_variant(z, cfg, dev, "double_target", _adam_check(z, cfg, "double_target"),
                              graph_learn=True)
    msgs = [w for w in caught if "learn-graph capture failed" in str(w.message)]
    assert len(msgs) == 1 and len(tries) == 1
    assert policy._graph_failed and not policy._learn_graphs


def test_sync_weight_is_one_copy_of_the_flat_storage(z, cfg, dev, monkeypatch):
    policy, _, _, buf = _updates(z, cfg, dev, "double_target", [32])
    fa = policy._flat
    flat, old = fa.flat_param, policy._old_flat
    lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * 4
    assert all(lo <= p.data_ptr() < hi for p in policy.model.parameters())
    assert len(fa.params) == 2 * (2 + 1 + 1 + 3 * 2)  # common 2, value 1 + 1, branches 3 x 2
    assert old is not None and old.shape == flat.shape and old.data_ptr() != lo
    storages = {p.untyped_storage().data_ptr() for p in policy.model_old.parameters()}
    assert storages == {old.untyped_storage().data_ptr()}
    policy.update(32, buf)  # _iter 1 of freq 2: no sync, the online network moved on
    assert not torch.equal(old, flat)
    copies, real = [], torch.Tensor.copy_
    policy.model_old.load_state_dict = None  # the fallback is not taken
    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "copy_",
                   lambda self, *a, **k: (copies.append(self), real(self, *a, **k))[1])
        policy.sync_weight()
    assert len(copies) == 1 and copies[0] is old and torch.equal(old, flat)
    assert not policy.model_old.training and policy.train().model.training


def test_other_optimisers_keep_torch_step(z, cfg, dev):
    policy, v = bh.make_policy(z, cfg, "double_target", dev)
    policy.optim = torch.optim.SGD(policy.model.parameters(), lr=1e-2)
    buf = _filled_buffer(z, cfg, "double_target", dev)
    before = [p.detach().clone() for p in policy.model.parameters()]
    np.random.seed(3)
    losses = [policy.update(v["bs"], buf)["loss"] for _ in range(3)]
    assert policy._flat is None or not policy._flat.adam_bound(policy.optim)
    assert not policy._learn_graphs
    assert all(np.isfinite(losses)) and len(set(losses)) == 3
    assert all(not torch.equal(a, b) for a, b in zip(before, policy.model.parameters()))


def test_switches_off_launch_none_of_the_new_kernels(z, cfg, dev, monkeypatch):
    policy, v = bh.make_policy(z, cfg, "double_target", dev, fused=False)
    policy.model.fused_combine = False
    policy.model_old.fused_combine = False
    buf = _filled_buffer(z, cfg, "double_target", dev)
    calls = _count_calls(monkeypatch)
    np.random.seed(3)
    losses = [policy.update(v["bs"], buf)["loss"] for _ in range(2)]
    assert calls == {} and all(np.isfinite(losses))
    policy.fused = True  # the policy's kernels alone
    policy.update(v["bs"], buf)
    assert set(calls) == {"tsrl_bdq_target", "tsrl_bdq_td_fwd_bwd"}


def test_foreign_network_gets_torch_argmax(dev):
    from tianshou_amd.data import Batch

    class Table(torch.nn.Module):
        num_branches, action_per_branch = 2, 3

        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.tensor([[1.0, 3.0, 3.0], [2.0, 2.0, 1.0]]))

        def forward(self, obs, state=None, **kw):
            return self.w[None].expand(len(obs), 2, 3) + 0.0, state

    p = BranchingDQNPolicy(Table().to(dev), None)
    out = p(Batch(obs=torch.zeros(4, 1, device=dev), info=Batch()))
    assert out.act.is_cuda and out.act.dtype == torch.int64 and out.act.shape == (4, 2)
    assert torch.equal(out.act, out.logits.max(dim=-1)[1])


def test_checkpoint_of_the_reference_loads_strictly(z, cfg, dev):
    from tianshou_amd.data import Batch
    policy, v = bh.make_policy(z, cfg, "double_target", dev)
    sd = {"model." + k: t for k, t in bh.init_state(z, "double_target_init_").items()}
    sd.update({"model_old." + k: t for k, t in bh.init_state(z, "double_target_init_").items()})
    assert set(policy.state_dict()) == set(sd)
    policy.load_state_dict(sd, strict=True)
    obs = torch.as_tensor(z["add_obs"][:9], device=dev)
    with torch.no_grad():
        out = policy(Batch(obs=obs, info=Batch()))
    want = bh.f64_forward({k: z["double_target_init_" + k] for k in policy.model.state_dict()},
                          z["add_obs"][:9], v["K"])
    np.testing.assert_allclose(out.logits.cpu().numpy(), want, rtol=1e-5, atol=1e-6)
    assert np.array_equal(out.act.cpu().numpy(), want.argmax(2))


# -- Collector and trainer --------------------------------------------------------------------------
def _collect_setup(z, dev):
    from tianshou_amd.data import Collector, VectorReplayBuffer
    from tianshou_amd.env import Box
    from tianshou_amd.env.synthetic import SyntheticVectorEnv
    from tianshou_amd.env.wrappers import ContinuousToDiscrete
    from tianshou_amd.utils.net import BranchingNet
    c = json.loads(str(z["col_cfg"]))
    E, D, K, A = c["E"], c["D"], c["K"], c["A"]
    base = SyntheticVectorEnv(E, (D,), K, ep_len=c["L"], seed=c["env_seed"], device=dev,
                              act_coef=c["act_coef"])
    base.action_space = Box(np.array(c["low"], np.float32), np.array(c["high"], np.float32),
                            (K,))
    env = ContinuousToDiscrete(base, A)
    net = BranchingNet(D, K, A, [16, 16], [8], [8], device=dev).to(dev)
    net.load_state_dict(bh.init_state(z, "col_init_"), strict=True)
    policy = BranchingDQNPolicy(net, torch.optim.Adam(net.parameters(), lr=1e-3),
                                target_update_freq=10).to(dev)
    policy.set_eps(c["eps"])
    buf = VectorReplayBuffer(c["size"], E, device=dev)
    return c, policy, buf, Collector(policy, env, buf, exploration_noise=True)


@pytest.mark.parametrize("graph_steps", (64, 0))
def test_collect_through_the_wrapper_matches_reference(z, dev, graph_steps):
    """(d) of the recording.  Half of the stored actions are NumPy's draws, the rest greedy
    with every per-branch top-two gap >= 1e-4 (asserted by the generator): equal.  Rewards,
    flags and episode statistics do not depend on the action: equal.  Observations carry
    f32(0.05 * mesh point): atol 5e-7, tests/test_gpu_ddpg.py's bound for this env."""
    c, policy, buf, col = _collect_setup(z, dev)
    col.graph_steps = graph_steps
    assert col._fused and col._noise_active() and col._act_spec() == ((c["K"],), torch.int64)
    assert float(c["min_gap"]) >= 1e-4
    np.random.seed(c["seed"])
    res = col.collect(n_step=c["n_step"])
    st = np.random.get_state()
    assert np.array_equal(st[1], z["col_state_keys"]) and st[2] == int(z["col_state_pos"])
    assert res["n/ep"] == int(z["col_n_ep"]) and res["n/st"] == int(z["col_n_st"])
    for k in ("lens", "idxs"):
        assert np.asarray(res[k]).tolist() == z["col_" + k].tolist(), k
    np.testing.assert_allclose(np.asarray(res["rews"]), z["col_rews"], rtol=1e-12)
    m = buf._meta
    got_act = m.act.cpu().numpy()
    assert got_act.dtype == np.int64 and got_act.shape == z["col_buf_act"].shape
    assert np.array_equal(got_act, z["col_buf_act"])
    assert len(np.unique(got_act)) == c["A"]
    for k in ("rew", "terminated", "truncated", "done"):
        got, want = getattr(m, k).cpu().numpy(), z["col_buf_" + k]
        assert got.shape == want.shape and np.array_equal(got.astype(want.dtype), want), k
    for k in ("obs", "obs_next"):
        got, want = getattr(m, k).cpu().numpy(), z["col_buf_" + k]
        assert got.shape == want.shape and float(np.abs(want).max()) < 4.0, k
        print(k, "max |obs - recorded|", float(np.abs(got - want).max()))
        np.testing.assert_allclose(got, want, rtol=0, atol=5e-7, err_msg=k)


def test_multi_discrete_synthetic_env_collects(dev):
    from tianshou_amd.data import Collector, VectorReplayBuffer
    from tianshou_amd.env.synthetic import SyntheticVectorEnv
    from tianshou_amd.utils.net import BranchingNet
    env = SyntheticVectorEnv(4, (5,), ep_len=7, device=dev, nvec=[3, 3])
    assert env.action_space.nvec.tolist() == [3, 3]
    with pytest.raises(AssertionError):
        SyntheticVectorEnv(4, (5,), 2, device=dev, act_coef=0.1, nvec=[3, 3])
    net = BranchingNet(5, 2, 3, [16], [8], [8], device=dev).to(dev)
    policy = BranchingDQNPolicy(net, torch.optim.Adam(net.parameters(), lr=1e-3)).to(dev)
    buf = VectorReplayBuffer(80, 4, device=dev)
    col = Collector(policy, env, buf)
    assert col.collect(n_step=40)["n/st"] == 40
    act = buf._meta.act[buf.sample_indices(0)]
    assert act.dtype == torch.int64 and act.shape == (40, 2) and int(act.max()) < 3
    assert col.collect(n_step=8, random=True)["n/st"] == 8


class _HostView:
    """A device vector env seen as a host one (NumPy in and out).  A prioritized buffer takes
    the Collector's generic loop, which reads host observations."""
    is_async = False

    def __init__(self, venv):
        self.venv, self.action_space = venv, venv.action_space

    def __len__(self):
        return len(self.venv)

    def reset(self, id=None, **kwargs):
        obs, _ = self.venv.reset(id)
        return obs.cpu().numpy(), [{} for _ in range(len(obs))]

    def step(self, action, id=None):
        obs, rew, term, trunc, _ = self.venv.step(action, id)
        ids = range(len(obs)) if id is None else np.atleast_1d(id)
        return (obs.cpu().numpy(), rew.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy(),
                np.array([{"env_id": int(j)} for j in ids]))


def test_offpolicy_trainer_runs_with_a_prioritized_buffer(z, dev):
    from tianshou_amd.data import Collector, PrioritizedVectorReplayBuffer
    from tianshou_amd.trainer import OffpolicyTrainer
    c, policy, _, _ = _collect_setup(z, dev)
    col_env = _HostView(_collect_setup(z, dev)[3].env)
    buf = PrioritizedVectorReplayBuffer(c["size"], c["E"], alpha=0.6, beta=0.4, device=dev)
    train = Collector(policy, col_env, buf, exploration_noise=True)
    test = Collector(policy, _collect_setup(z, dev)[3].env)
    np.random.seed(1)
    train.collect(n_step=32)
    losses = []
    learn = policy.learn

    def rec_learn(batch, **kw):
        res = learn(batch, **kw)
        losses.append(res["loss"])
        return res

    policy.learn = rec_learn
    result = OffpolicyTrainer(policy, max_epoch=2, batch_size=16, train_collector=train,
                              test_collector=test, step_per_epoch=24, step_per_collect=8,
                              episode_per_test=2, update_per_step=0.25,
                              train_fn=lambda e, s: policy.set_eps(0.3),
                              test_fn=lambda e, s: policy.set_eps(0.0), verbose=False,
                              show_progress=False, test_in_train=False).run()
    assert len(losses) == 2 * 3 * 2 and all(np.isfinite(losses))
    assert policy._iter == len(losses) and result["best_reward"] is not None
