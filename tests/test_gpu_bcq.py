"""csrc/bcq.hip through the C ABI, and BCQPolicy on the device path.

tsrl_group_linear against an f64 cat + matmul: the max-norm error may be at most four times
that of torch's own f32 cat + F.linear on the same inputs on the same GPU (the allowance of the
Fisher product and the IQN embedding), canary rows after ``out`` intact.  The per-element
kernels against torch f64 (tests/bcq_common.py): loss scalars rtol 1e-5, gradients rtol 1e-4
with atol 1e-6 * max|ref|; forward values (z, std, the perturbed action, the target) are a few
f32 roundings of their largest operand: rtol 1e-5 with the same atol.

Policies: the recorded updates of tests/golden/bcq.npz (the reference on CPU torch) on the
default (graph replay, dense learn), graph, eager, no-group and torch legs: sampled indices equal, losses rtol 2e-5 / atol 1e-6,
parameters online and target rtol 1e-5 / atol 1e-6, forward's actions; graph replay equals the
eager leg bitwise."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bcq_common as bc
from tianshou_amd import _C
from tianshou_amd.data.batch import Batch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KERNELS = ("tsrl_group_linear", "tsrl_bcq_vae_sample_fwd", "tsrl_bcq_vae_sample_bwd",
           "tsrl_bcq_vae_loss_fwd_bwd", "tsrl_bcq_perturb_fwd", "tsrl_bcq_perturb_bwd",
           "tsrl_bcq_target", "tsrl_bcq_select_act")


def _d(x):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV)


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _parts(rows, k):
    return _nan(k * int(_C.lib().tsrl_ddpg_num_partials(rows)), dtype=torch.float64)


def _close(got, want, tag, rtol=1e-4):
    want = np.asarray(want, np.float64)
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=rtol,
                               atol=1e-6 * float(np.max(np.abs(want))), err_msg=tag)


def _call(name, *args):
    _C.check(getattr(_C.lib(), name)(*(_C.ptr(a) if isinstance(a, torch.Tensor) else a
                                       for a in args), _C.stream_ptr(DEV)), name)


# -- tsrl_group_linear ----------------------------------------------------------------------------
def _group_inputs(G, R, D, K, H, n_out):
    g = np.random.default_rng(G + 10 * R + D + K + H)
    xs, xo = g.normal(size=(G, D)).astype(np.float32), g.normal(size=(G * R, K)).astype(np.float32)
    layers = [(g.normal(size=(H, D + K)).astype(np.float32) / np.float32(np.sqrt(D + K)),
               g.normal(size=H).astype(np.float32)) for _ in range(n_out)]
    return xs, xo, layers


def _group_run(xs, xo, layers, R, relu, canary=2):
    (G, D), K, H = xs.shape, xo.shape[1], layers[0][0].shape[0]
    bufs = [_nan(G * R + canary, H) for _ in layers]
    dev, txs, txo = [(_d(w), _d(b)) for w, b in layers], _d(xs), _d(xo)
    second = (dev[1][0].data_ptr(), dev[1][1].data_ptr(), bufs[1].data_ptr()) \
        if len(layers) == 2 else (None, None, None)
    rc = _C.lib().tsrl_group_linear(
        _C.ptr(txs), _C.ptr(txo), _C.ptr(dev[0][0]), D + K, _C.ptr(dev[0][1]),
        _C.ptr(bufs[0]), *second, G, R, D, K, H, relu, _C.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc, bufs


@pytest.mark.parametrize("G,R,D,K,H,relu,dual", bc.GROUP_CASES)
def test_group_linear_matches_f64(G, R, D, K, H, relu, dual):
    xs, xo, layers = _group_inputs(G, R, D, K, H, 2 if dual else 1)
    rc, bufs = _group_run(xs, xo, layers, R, relu)
    assert rc == 0, _C.lib().tsrl_last_error()
    if (G, R) == (1, 100):
        assert _C.lib().tsrl_group_linear_splits(G, R, D, K, H, 1) > 1
    x32 = torch.cat([_d(xs).repeat_interleave(R, 0), _d(xo)], -1)
    for (w, b), buf in zip(layers, bufs):
        want = x32.double() @ _d(w).double().T + _d(b).double()
        mine, theirs = buf[:G * R], F.linear(x32, _d(w), _d(b))
        if relu:
            want, theirs = want.clamp_min(0), theirs.clamp_min(0)
        e_mine = float((mine.double() - want).abs().max())
        e_torch = float((theirs.double() - want).abs().max())
        print(f"group_linear {(G, R, D, K, H)}: error {e_mine:.3e}, torch f32 {e_torch:.3e}")
        assert e_mine <= 4 * e_torch
        assert torch.isnan(buf[G * R:]).all()  # the canary rows


def test_group_linear_declines_a_wide_own_block():
    K = _C.GROUP_LINEAR_MAX_OWN + 1
    xs, xo, layers = _group_inputs(3, 2, 5, K, 8, 1)
    rc, bufs = _group_run(xs, xo, layers, 2, 1)
    assert rc == _C.ERR_GROUP_LINEAR_SHAPE and b"exceeds" in _C.lib().tsrl_last_error()
    assert torch.isnan(bufs[0]).all()


def test_grouped_first_layer_opens_the_nets():
    """An MLP, a Net and a pair of Critics over a Net take the kernel and agree with their own
    forward over repeat + cat; a norm layer after the first Linear falls back to those lines."""
    from tianshou_amd.utils import net as N
    G, R, D, K = 5, 3, 7, 2
    torch.manual_seed(0)
    xs, xo = torch.randn(G, D, device=DEV), torch.randn(G * R, K, device=DEV)
    x = torch.cat([xs.repeat_interleave(R, 0), xo], -1)
    nets = [N.MLP(D + K, 4, (8,), device=DEV).to(DEV), N.Net(D + K, 4, (8,), device=DEV).to(DEV),
            N.MLP(D + K, 4, (8,), norm_layer=torch.nn.LayerNorm, device=DEV).to(DEV)]
    critics = tuple(N.Critic(N.Net(D, K, (8,), concat=True, device=DEV), device=DEV).to(DEV)
                    for _ in range(2))
    calls, L, real = [], _C.lib(), _C.lib().tsrl_group_linear
    L.tsrl_group_linear = lambda *a: (calls.append(a[6]), real(*a))[1]
    try:
        with torch.no_grad():
            for n in nets:
                got, want = N.grouped_first_layer(n, xs, xo, R), n(x)
                got, want = (t[0] if isinstance(t, tuple) else t for t in (got, want))
                torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6)
            assert len(calls) == 2
            for got, c in zip(N.grouped_first_layer(critics, xs, xo, R), critics):
                torch.testing.assert_close(got, c(x), rtol=1e-5, atol=1e-6)
        assert len(calls) == 3 and calls[2] is not None  # the pair: one launch, two outputs
    finally:
        L.tsrl_group_linear = real


# -- the per-element kernels ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("interior", "upper"))
@pytest.mark.parametrize("A", (1, 6))
@pytest.mark.parametrize("b", (1, 255, 257))
def test_vae_kernels_match_f64(b, A, kind):
    """Each output against the bound of its own magnitude (bcq_common.vae_case keeps the
    std = e^15 rows out of the ordinary case); each loss scalar on its own, rtol 1e-5."""
    L, c = 2 * A, bc.vae_case(kind, b, A)
    (want_z, want_std, _), want_loss, (g_recon, g_mean, g_ls) = bc.vae_ref(**c)
    m, ls, e, wd = (_d(c[k]) for k in ("mean", "log_std", "noise", "wd"))
    z, std = _nan(b, L), _nan(b, L)
    _call("tsrl_bcq_vae_sample_fwd", m, ls, e, b * L, z, std)
    _close(z, want_z, "z", 1e-5)
    _close(std, want_std, "std", 1e-5)
    recon = (z.double() @ wd).float()
    g_r, loss = _nan(b, A), _nan(3)
    _call("tsrl_bcq_vae_loss_fwd_bwd", _d(c["act"]), recon, m, std, b, A, L, g_r, _parts(b, 2),
          loss)
    np.testing.assert_allclose(loss.cpu().numpy(), want_loss, rtol=1e-5, atol=0)
    _close(g_r, g_recon, "g_recon")
    g_z = (g_r.double() @ wd.T).float()
    gm, gl = _nan(b, L), _nan(b, L)
    _call("tsrl_bcq_vae_sample_bwd", g_z, m, ls, e, std, b * L, gm, gl)
    _close(gm, g_mean, "g_mean")
    _close(gl, g_ls, "g_log_std")
    outside = (c["log_std"] < -4) | (c["log_std"] > 15)
    assert outside.any() == (kind == "interior" or b * L > 2)
    assert (gl.cpu().numpy()[outside] == 0).all()
    assert (gl.cpu().numpy()[~outside] != 0).all()  # equality passes the gradient


@pytest.mark.parametrize("stride0", (False, True))
@pytest.mark.parametrize("A", (1, 6))
@pytest.mark.parametrize("b", (1, 255, 257))
def test_perturb_matches_f64(b, A, stride0):
    g = np.random.default_rng(10 * b + A)
    m, phi = 1.5, 0.05
    logits = g.normal(size=(A,) if stride0 else (b, A)).astype(np.float32)
    act = g.uniform(-1.2 * m, 1.2 * m, (b, A)).astype(np.float32)
    act.flat[:2] = (m + 0.5, -m - 0.5)[:b * A]  # beyond the bounds
    if not stride0 and b * A >= 4:  # exactly at them: tanh(0) = 0
        logits.flat[2:4], act.flat[2:4] = 0.0, (m, -m)
    g_out = g.normal(size=(b, A)).astype(np.float32)
    want, want_gl, want_ga = bc.perturb_ref(logits, act, phi, m, g_out)
    lg, a, out = _d(logits), _d(act), _nan(b, A)
    ls = 0 if stride0 else A
    _call("tsrl_bcq_perturb_fwd", lg, ls, a, phi, m, b, A, out)
    _close(out, want, "out", 1e-5)
    g_a, g_l = _nan(b, A), _nan(*logits.shape)
    _call("tsrl_bcq_perturb_bwd", _d(g_out), lg, ls, a, phi, m, b, A, g_a, g_l,
          _parts(b, A) if stride0 else None)
    _close(g_a, want_ga, "g_act")
    _close(g_l, want_gl, "g_logits")
    assert g_a.flatten()[0] == 0 and (b * A < 4 or stride0 or (g_a.flatten()[2:4] != 0).all())


@pytest.mark.parametrize("lmbda", (0.0, 0.75, 1.0))
@pytest.mark.parametrize("R", (1, 10))
@pytest.mark.parametrize("b", (1, 255, 257))
def test_target_matches_f64(b, R, lmbda):
    g = np.random.default_rng(b + R)
    q1, q2 = (g.normal(size=b * R).astype(np.float32) * 3 for _ in range(2))
    q2[::3] = q1[::3]
    rew = g.normal(size=b).astype(np.float32)
    done = (g.random(b) < 0.4).astype(np.float32)
    done[0] = 1.0
    out = _nan(b)
    _call("tsrl_bcq_target", _d(q1), _d(q2), _d(rew), _d(done), lmbda, 0.97, b, R, out)
    _close(out, bc.target_ref(q1, q2, rew, done, lmbda, 0.97, R), "target", 1e-5)
    assert out[0].item() == rew[0]


@pytest.mark.parametrize("A", (1, 6))
@pytest.mark.parametrize("G,R", ((1, 1), (3, 10), (257, 10), (10, 100)))
def test_select_takes_the_first_maximum(G, R, A):
    g = np.random.default_rng(G + R + A)
    q = g.normal(size=(G, R)).astype(np.float32)
    if R > 1:  # an exact tie at the top of group 0: the first index wins
        q[0, [R // 2, R - 1]] = 10.0
    act = g.normal(size=(G * R, A)).astype(np.float32)
    out, idx = _nan(G, A), torch.full((G,), -1, dtype=torch.int64, device=DEV)
    _call("tsrl_bcq_select_act", _d(q), _d(act), G, R, A, out, idx)
    want = torch.as_tensor(q).argmax(1).numpy()
    assert idx.cpu().numpy().tolist() == want.tolist() and (R == 1 or want[0] == R // 2)
    np.testing.assert_array_equal(out.cpu().numpy(), act.reshape(G, R, A)[np.arange(G), want])


# -- policies against tests/golden/bcq.npz ----------------------------------------------------------
LEGS = {"default": {},  # what ships: graph replay, the grouped layer in forward alone
        "graph": dict(graph_learn=True, fused_group_learn=True),
        "eager": dict(graph_learn=False, fused_group_learn=True),
        "nogroup": dict(graph_learn=False, fused_group=False), "torch": dict(fused=False)}


@functools.lru_cache(maxsize=None)
def _run_leg(golden_dir, tag, leg):
    """The recorded updates and the forward on one leg, every result checked against the
    recording; returns (losses, final state, actions, kernel calls) for the comparisons."""
    from tianshou_amd.data import VectorReplayBuffer
    z, cfg = bc.recording(golden_dir)
    calls, L = [], _C.lib()
    real = {s: getattr(L, s) for s in KERNELS}
    for s, f in real.items():
        setattr(L, s, (lambda f, s: lambda *a: (calls.append(s), f(*a))[1])(f, s))
    try:
        policy = bc.make_policy(z, cfg, tag, DEV, **LEGS[leg])
        policy.train()
        bc.feed_draws(policy, z, tag, cfg["updates"])
        buf = VectorReplayBuffer(cfg["E"] * cfg["S"], cfg["E"], device=DEV)
        o = 0
        for k in z["add_len"]:
            sl = slice(o, o + int(k))
            buf.add(Batch(**{key: z["add_" + key][sl] for key in (
                "obs", "act", "rew", "terminated", "truncated", "obs_next")}),
                buffer_ids=z["add_ids"][sl])
            o += int(k)
        process_fn, seen, losses = policy.process_fn, [], []
        policy.process_fn = lambda b, bf, i: (seen.append(np.array(i, copy=True)),
                                              process_fn(b, bf, i))[1]
        np.random.seed(cfg["sample_seed"])
        for u in range(cfg["updates"]):
            res = policy.update(cfg["bs"], buf)
            assert seen[u].tolist() == z[f"{tag}_u{u}_indices"].tolist()
            bc.check_update(policy, z, tag, u, res)
            losses.append(list(res.values()))
        policy.eval()
        act = policy(Batch(obs=torch.as_tensor(z["fixed_obs"], device=DEV), info=Batch())).act
        act = act.cpu().numpy() if isinstance(act, torch.Tensor) else act
        np.testing.assert_allclose(act, z[tag + "_fixed_act"], rtol=1e-5, atol=1e-6)
        assert bool(policy._learn_graphs) == (leg in ("default", "graph"))
        assert not policy._graph_failed
        sd = {k: t.detach().cpu().clone() for k, t in policy.state_dict().items()}
        return losses, sd, act, calls
    finally:
        for s, f in real.items():
            setattr(L, s, f)


@pytest.mark.parametrize("leg", tuple(LEGS))
@pytest.mark.parametrize("tag", ("example", "net", "single"))
def test_update_and_forward_match_reference(golden_dir, tag, leg):
    calls = _run_leg(golden_dir, tag, leg)[3]
    if leg == "torch":
        assert not calls
    else:  # the group kernel runs on its legs alone; a replayed update makes no call
        assert ("tsrl_group_linear" in calls) == (leg != "nogroup")
        assert calls.count("tsrl_bcq_target") == (2 if leg in ("default", "graph") else 4)
        # forward launches it three times; learn twice per update made outside a replay
        assert calls.count("tsrl_group_linear") == {"default": 3, "graph": 7, "eager": 11,
                                                    "nogroup": 0}[leg]
        assert calls.count("tsrl_bcq_select_act") == 1


@pytest.mark.parametrize("tag", ("example", "net", "single"))
def test_graph_replay_equals_eager_bitwise(golden_dir, tag):
    graph, eager = (_run_leg(golden_dir, tag, leg) for leg in ("graph", "eager"))
    assert graph[0] == eager[0]
    assert all(torch.equal(graph[1][k], eager[1][k]) for k in eager[1])
    np.testing.assert_array_equal(graph[2], eager[2])


def test_offline_trainer_runs_bcq_on_the_device_path(golden_dir):
    from tianshou_amd.data import Collector, VectorReplayBuffer
    from tianshou_amd.env import SyntheticVectorEnv
    from tianshou_amd.trainer import OfflineTrainer
    z, cfg = bc.recording(golden_dir)
    p, E, D, A = bc.make_policy(z, cfg, "example", DEV), 4, cfg["D"], cfg["A"]
    buf = VectorReplayBuffer(E * 64, E, device=DEV)
    Collector(p, SyntheticVectorEnv(E, (D,), A, ep_len=16, device=DEV), buf).collect(
        n_step=E * 48)
    test_c = Collector(p, SyntheticVectorEnv(2, (D,), A, ep_len=16, seed=5, device=DEV))
    tr = OfflineTrainer(p, buffer=buf, test_collector=test_c, max_epoch=2, step_per_epoch=4,
                        episode_per_test=2, batch_size=32, verbose=False, show_progress=False)
    info = tr.run()
    assert tr.gradient_step == 8 and "best_reward" in info and p._learn_graphs
