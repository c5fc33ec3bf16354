"""csrc/offline_cont.hip through the C ABI, and CQLPolicy / TD3BCPolicy on the device path.

Kernels, outputs into NaN-prefilled buffers: tsrl_cql_expand exactly; tsrl_cql_target bitwise
against torch's f32 formulation (tests/test_gpu_sac.py's rule for tsrl_sac_target); the TD3+BC
loss and the CQL kernel's q gradients at tsrl_sac_actor_loss_fwd_bwd's bounds there (scalars
rtol 1e-5, gradients rtol 1e-4 with atol 1e-6 * max|ref|).  The three-way logsumexp terms (the
CQL losses, g_v and the multiplier's gradient) are held to four times what torch's f32
formulation deviates from f64 on the same inputs, measured on the CPU over every case below:
losses at most 2.5e-7 of the largest |loss| of the case, g_v at most 1.0e-6 (1.9e-5 in the
case with values near 1e3 / temperature, where f32 rounds the exponent itself) and the
multiplier's gradient at most 2.2e-7, relative to the largest |ref| -- LSE_LOSS, LSE_GRAD,
LSE_GRAD_1E3, LSE_MULT.

Policies: the recorded updates of tests/golden/cont_offline.npz (the reference on CPU torch) on
the graph, eager and torch legs: sampled indices equal, losses rtol 2e-5 / atol 1e-6, Adam
parameters online and target, the temperature and the multiplier rtol 1e-5 / atol 1e-6."""
import numpy as np
import pytest
import torch

from tests import cont_offline_common as cc
from tianshou_amd import _C
from tianshou_amd.data.batch import Batch

pytestmark = pytest.mark.gpu
LSE_LOSS, LSE_GRAD, LSE_GRAD_1E3, LSE_MULT = 4 * 2.5e-7, 4 * 1.0e-6, 4 * 1.9e-5, 4 * 2.2e-7
LAGRANGE = {"off": None, "inside": (0.0, 1e6), "below": (2.0, 1e6), "above": (0.0, 0.9)}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _d(x, dev):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), device=dev)


def _nan(dev, *shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _parts(rows, k, dev):
    return _nan(dev, k * int(_C.lib().tsrl_ddpg_num_partials(rows)), dtype=torch.float64)


def _close(got, want, tag, rtol=1e-4):
    want = np.asarray(want)
    atol = 1e-6 * float(np.max(np.abs(want))) if rtol == 1e-4 else 0.0
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=rtol, atol=atol, err_msg=tag)


@pytest.mark.parametrize("b,R,D,A", ((1, 1, 1, 1), (3, 10, 5, 2), (7, 4, 8, 6), (26, 10, 17, 3)))
def test_expand_is_exact(dev, b, R, D, A):
    """D = 8 takes the 16-byte path, the others (and an obs view one float off alignment) the
    scalar one; 26 * 10 rows of 17 floats span several workgroups."""
    g = np.random.default_rng(b + D)
    obs, nxt = (g.normal(size=(b, D)).astype(np.float32) for _ in range(2))
    u = g.random((b * R, A), dtype=np.float32)
    lo, hi, n = 0.5, 1.25, b * R
    want_act = (np.float32(lo) + u * np.float32(hi - lo)).astype(np.float32)
    for shift in (0, 1):
        pad = [torch.zeros(b * D + 1, device=dev) for _ in range(2)]
        t = [p[shift:shift + b * D].view(b, D).copy_(_d(x, dev)) for p, x in zip(pad, (obs, nxt))]
        actor_in, c_obs, c_act = _nan(dev, 2 * n, D), _nan(dev, 3 * n, D), _nan(dev, 3 * n, A)
        ud = _d(u, dev)
        _C.check(_C.lib().tsrl_cql_expand(
            _C.ptr(t[0]), _C.ptr(t[1]), _C.ptr(ud), lo, hi, b, R, D, A, _C.ptr(actor_in),
            _C.ptr(c_obs), _C.ptr(c_act), _C.stream_ptr(dev)), "tsrl_cql_expand")
        rep, rep_next = np.repeat(obs, R, 0), np.repeat(nxt, R, 0)
        np.testing.assert_array_equal(actor_in.cpu().numpy(), np.concatenate([rep, rep_next]))
        np.testing.assert_array_equal(c_obs.cpu().numpy(), np.concatenate([rep] * 3))
        np.testing.assert_array_equal(c_act[:n].cpu().numpy(), want_act)
        assert torch.isnan(c_act[n:]).all()  # the sampled actions' rows are not touched


@pytest.mark.parametrize("b", (1, 255, 257))
def test_target_matches_torch_f32_bitwise(dev, b):
    g = np.random.default_rng(b)
    q1, q2, lp, rew = (g.normal(size=b).astype(np.float32) for _ in range(4))
    done = (g.random(b) < 0.4).astype(np.float32)
    done[0], q1[b // 2] = 0.0, np.nan
    alpha, gamma = np.float32(0.37), 0.97
    t = [torch.as_tensor(x) for x in (q1, q2, lp, rew, done)]
    want = t[3] + gamma * (1 - t[4]) * (torch.min(t[0], t[1]) - float(alpha) * t[2])
    out = _nan(dev, b)
    td = [_d(x, dev) for x in (q1, q2, lp, np.array([alpha]), rew, done)]
    _C.check(_C.lib().tsrl_cql_target(*(_C.ptr(x) for x in td), gamma, b, _C.ptr(out),
                                      _C.stream_ptr(dev)), "tsrl_cql_target")
    np.testing.assert_array_equal(out.cpu().numpy(), want.numpy())
    assert bool(torch.isnan(want[b // 2])) and (done > 0).any() == (b > 1)


def loss_case(b, R, A, T, mode, scale=2.0):
    g = np.random.default_rng(1000 * b + 10 * R + A)
    n = b * R
    c = dict(q1=g.normal(size=b) * 2, q2=g.normal(size=b) * 2, target=g.normal(size=b),
             v1=g.normal(size=(3, n)) * scale, v2=g.normal(size=(3, n)) * scale,
             log_pi=g.normal(size=(2, n)) - 1.0, log_alpha=np.array([0.3]))
    c = {k: x.astype(np.float32) for k, x in c.items()}
    amin, amax = LAGRANGE[mode] or (0.0, 1e6)
    return c, dict(T=T, w=1.5, thr=2.0, amin=amin, amax=amax, A=A, lagrange=mode != "off")


def check_cql_loss(case, kw, b, R, got, grad_tol=LSE_GRAD):
    """``got``: (losses [4] (NaN without the multiplier), [g_q1, g_q2, g_v1, g_v2], g_la)."""
    want, grads, g_la = cc.cql_ref(**case, **kw)
    k = 4 if kw["lagrange"] else 2
    scale = float(np.max(np.abs(want[:k])))
    np.testing.assert_allclose(got[0][:k], np.array(want[:k], np.float64).ravel(), rtol=0,
                               atol=LSE_LOSS * scale)
    for i in (0, 1):
        _close(got[1][i], grads[i], f"g_q{i + 1}")
        ref = grads[2 + i].ravel()
        np.testing.assert_allclose(got[1][2 + i].cpu().numpy(), ref, rtol=0,
                                   atol=grad_tol * float(np.abs(ref).max()))
    if kw["lagrange"]:
        inside = kw["amin"] <= np.exp(np.float32(0.3)) <= kw["amax"]
        assert (g_la != 0).all() == inside
        ref = np.abs(cc.cql_ref(**case, **dict(kw, amin=0.0, amax=1e6))[2]).max()
        np.testing.assert_allclose(got[2], g_la, rtol=0, atol=LSE_MULT * float(ref))
    else:
        assert np.isnan(got[0][2:]).all() and np.isnan(got[2]).all()


def run_cql_loss(case, kw, b, R, dev):
    n = b * R
    t = {k: _d(x, dev) for k, x in case.items()}
    grads = [_nan(dev, b), _nan(dev, b), _nan(dev, 3 * n), _nan(dev, 3 * n)]
    loss, lag, g_la, parts = _nan(dev, 2), _nan(dev, 2), _nan(dev, 1), _parts(n, 6, dev)
    _C.check(_C.lib().tsrl_cql_loss_fwd_bwd(
        *(_C.ptr(t[k]) for k in ("q1", "q2", "target", "v1", "v2", "log_pi", "log_alpha")),
        kw["T"], kw["w"], kw["thr"], kw["amin"], kw["amax"], kw["A"], int(kw["lagrange"]), b, R,
        *(_C.ptr(x) for x in grads), _C.ptr(parts), _C.ptr(loss), _C.ptr(lag), _C.ptr(g_la),
        _C.stream_ptr(dev)), "tsrl_cql_loss_fwd_bwd")
    return torch.cat([loss, lag]).cpu().numpy().astype(np.float64), grads, g_la.cpu().numpy()


@pytest.mark.parametrize("mode", tuple(LAGRANGE))
@pytest.mark.parametrize("T", (1.0, 0.5))
@pytest.mark.parametrize("A", (1, 6))
@pytest.mark.parametrize("b,R", ((1, 1), (3, 10), (26, 10), (256, 1), (257, 2)))
def test_cql_loss_matches_f64(dev, b, R, A, T, mode):
    case, kw = loss_case(b, R, A, T, mode)
    check_cql_loss(case, kw, b, R, run_cql_loss(case, kw, b, R, dev))


def test_cql_loss_subtracts_the_maximum(dev):
    """Values near 1e3 / temperature: exp of an unsubtracted value overflows f32 and f64."""
    case, kw = loss_case(26, 10, 6, 0.5, "inside", scale=1e3)
    assert np.abs(case["v1"]).max() / 0.5 > 710
    check_cql_loss(case, kw, 26, 10, run_cql_loss(case, kw, 26, 10, dev), LSE_GRAD_1E3)


@pytest.mark.parametrize("A", (1, 6))
@pytest.mark.parametrize("b", (1, 256, 257))
def test_td3bc_actor_loss_matches_f64(dev, b, A):
    g = np.random.default_rng(b + A)
    q = (g.normal(size=b) * 3 + 1).astype(np.float32)
    act, data = (g.uniform(-1, 1, (b, A)).astype(np.float32) for _ in range(2))
    g_q, g_act, loss = _nan(dev, b), _nan(dev, b, A), _nan(dev, 1)
    t = [_d(x, dev) for x in (q, act, data)] + [_parts(b, 3, dev)]
    _C.check(_C.lib().tsrl_td3bc_actor_loss_fwd_bwd(
        _C.ptr(t[0]), _C.ptr(t[1]), _C.ptr(t[2]), 2.5, b, A, _C.ptr(g_q), _C.ptr(g_act),
        _C.ptr(t[3]), _C.ptr(loss), _C.stream_ptr(dev)), "tsrl_td3bc_actor_loss_fwd_bwd")
    want, want_gq, want_ga = cc.td3bc_ref(q, act, data, 2.5)
    _close(loss, [want], "loss", rtol=1e-5)
    _close(g_q, want_gq, "g_q")
    _close(g_act, want_ga, "g_act")


# -- policies against tests/golden/cont_offline.npz ------------------------------------------------
LEGS = {"graph": dict(graph_learn=True), "eager": dict(graph_learn=False),
        "torch": dict(fused=False)}


@pytest.mark.parametrize("leg", tuple(LEGS))
@pytest.mark.parametrize("tag", ("cql_lagrange", "cql_clamped", "cql_plain", "td3bc"))
def test_update_matches_reference(golden_dir, dev, tag, leg, monkeypatch):
    from tianshou_amd.data import VectorReplayBuffer
    z, cfg = cc.recording(golden_dir)
    calls, L = [], _C.lib()
    for s in ("tsrl_cql_expand", "tsrl_cql_target", "tsrl_cql_loss_fwd_bwd",
              "tsrl_td3bc_actor_loss_fwd_bwd"):
        monkeypatch.setattr(L, s, (lambda f, s=s: lambda *a: (calls.append(s), f(*a))[1])(
            getattr(L, s)))
    policy, v = cc.make_policy(z, cfg, tag, dev, **LEGS[leg]), cfg["variants"][tag]
    policy.train()
    cc.feed_draws(policy, z, tag, cfg["updates"])
    buf = VectorReplayBuffer(cfg["E"] * cfg["S"], cfg["E"], device=dev)
    o = 0
    for k in z["add_len"]:
        sl = slice(o, o + int(k))
        buf.add(Batch(**{key: z["add_" + key][sl] for key in (
            "obs", "act", "rew", "terminated", "truncated", "obs_next")}),
            buffer_ids=z["add_ids"][sl])
        o += int(k)
    process_fn, seen = policy.process_fn, []
    policy.process_fn = lambda b, bf, i: (seen.append(np.array(i, copy=True)),
                                          process_fn(b, bf, i))[1]
    np.random.seed(cfg["sample_seed"])
    for u in range(cfg["updates"]):
        res = policy.update(v["bs"], buf)
        assert seen[u].tolist() == z[f"{tag}_u{u}_indices"].tolist()
        cc.check_update(policy, z, tag, u, res, 2e-5)
    policy.eval()
    act = policy(Batch(obs=torch.as_tensor(z["fixed_obs"], device=dev), info=Batch())).act
    np.testing.assert_allclose(act.detach().cpu().numpy(), z[tag + "_fixed_act"], rtol=1e-5, atol=1e-6)
    if leg == "torch":
        assert not calls
        return
    assert bool(policy._learn_graphs) == (leg == "graph") and not policy._graph_failed
    n = cfg["updates"]
    if tag == "td3bc":  # actor steps at updates 0, 2, 4; replays make no call
        assert len(calls) == (2 if leg == "graph" else 3)
    else:  # a replayed update makes no call: the warm-up update and the capture do
        assert calls.count("tsrl_cql_loss_fwd_bwd") == (2 if leg == "graph" else n)
        assert calls.count("tsrl_cql_expand") == calls.count("tsrl_cql_target") == \
            calls.count("tsrl_cql_loss_fwd_bwd")


def test_offline_trainer_runs_cql_on_the_device_path(golden_dir, dev):
    from tianshou_amd.data import Collector, VectorReplayBuffer
    from tianshou_amd.env import SyntheticVectorEnv
    from tianshou_amd.trainer import OfflineTrainer
    z, cfg = cc.recording(golden_dir)
    p, E, D, A = cc.make_policy(z, cfg, "cql_lagrange", dev), 4, cfg["D"], cfg["A"]
    buf = VectorReplayBuffer(E * 64, E, device=dev)
    Collector(p, SyntheticVectorEnv(E, (D,), A, ep_len=16, device=dev), buf).collect(
        n_step=E * 48)
    test_c = Collector(p, SyntheticVectorEnv(2, (D,), A, ep_len=16, seed=5, device=dev))
    tr = OfflineTrainer(p, buffer=buf, test_collector=test_c, max_epoch=2, step_per_epoch=4,
                        episode_per_test=2, batch_size=32, verbose=False, show_progress=False)
    info = tr.run()
    assert tr.gradient_step == 8 and "best_reward" in info and p._learn_graphs
