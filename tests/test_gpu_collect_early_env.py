"""The fused collect step (csrc/collect.hip) at the shapes where a different placement of its env
phase could go wrong: the step's box_m hashes computed ahead of the deferred obs_rms merge and
staged in LDS, or the rows of a column split between its column thread and the spare threads
of the workgroup.  (Both were built and measured slower than the kernel's present form, see
the kernel's header; the cases stay as the fence for the next attempt.)

Every case runs the fused step against the four-launch step (``use_fused_step = False``) under
the asserts of tests/test_gpu_collect_step.py (test_fused_step_matches_four_launch_step, or
test_fused_step_action_coupled_env for the action-coupled env), and for the default env also
checks what such a split could break silently: the obs_rms moments are exact integer sums, so
two fused runs, and fused runs with ``graph_steps`` 0 and 4, give the same bits everywhere.

The shapes walk the thread split (D against NT = 512 threads and the R = 16 key threads), the
partial row tiles, resets on every launch and the chain structure (first launch without a
merge, the three-slot totals ring wrapping, a remainder graph, the closing plain add).  Every
listed D takes the fused path: Collector._fused_step_ok refuses only D > 512, and the helper
asserts ``c._step_on == fused``, so a fall-back fails the test."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _run(dev, fused, E, D, A, L, T, graph_steps, collects=1, act_coef=0.0):
    from tianshou_amd.data import Collector, VectorReplayBuffer
    from tianshou_amd.env import Box, SyntheticVectorEnv, VectorEnvNormObs
    from tianshou_amd.policy import PPOPolicy
    from tianshou_amd.utils.models import fixed_std_normal, get_actor_critic, init_and_get_optim
    torch.manual_seed(0)
    actor, critic = get_actor_critic((D,), (64, 64), (A,), dev)
    optim = init_and_get_optim(actor.to(dev), critic.to(dev), 3e-4)
    with torch.no_grad():
        for p in actor.parameters():
            p.add_(0.05 * torch.randn_like(p))
    pol = PPOPolicy(actor, critic, optim, fixed_std_normal,
                    action_space=Box(-2.0, 3.0, (A,)), action_bound_method="clip").to(dev)
    env = VectorEnvNormObs(SyntheticVectorEnv(E, (D,), A, ep_len=L, seed=5, device=dev,
                                              act_coef=act_coef))
    buf = VectorReplayBuffer(E * T * collects, E, device=dev)
    c = Collector(pol, env, buf)
    c.use_fused_step = fused
    c.graph_steps = graph_steps
    torch.manual_seed(1)
    res = []
    for _ in range(collects):
        res.append(c.collect(n_step=E * T))
        assert c._step_on == fused
    assert c._pending is None
    m = buf._meta
    out = {k: getattr(m, k).detach().cpu().clone() for k in
           ("obs", "obs_next", "act", "rew", "terminated", "truncated", "done")}
    out["env_id"] = m.info.env_id.cpu().clone()
    rms = env.obs_rms
    out["rms"] = (rms.mean_t.cpu().clone(), rms.var_t.cpu().clone(), rms.count)
    out["cur"] = c.data.obs.cpu().clone()
    d = buf._dev
    out["stats"] = [d[k].cpu().clone() for k in ("stat_rew", "stat_len", "stat_idx", "ep_rew",
                                                 "ep_len", "ep_idx")]
    return out, res


def _assert_bit_equal(a, ra, b, rb, what):
    for k in ("obs", "obs_next", "act", "rew", "terminated", "truncated", "done", "env_id",
              "cur"):
        assert torch.equal(a[k], b[k]), (what, k)
    assert torch.equal(a["rms"][0], b["rms"][0]), (what, "mean")
    assert torch.equal(a["rms"][1], b["rms"][1]), (what, "var")
    assert a["rms"][2] == b["rms"][2], (what, "count")
    for x, y in zip(a["stats"], b["stats"]):
        assert torch.equal(x, y), what
    for x, y in zip(ra, rb):
        assert x["n/ep"] == y["n/ep"] and x["n/st"] == y["n/st"], what
        assert np.array_equal(x["rews"], y["rews"]) and np.array_equal(x["lens"], y["lens"])
        assert np.array_equal(x["idxs"], y["idxs"])


def _assert_matches_four_launch(a, ra, b, rb):
    """test_fused_step_matches_four_launch_step's asserts."""
    for k in ("rew", "terminated", "truncated", "done", "env_id"):
        assert torch.equal(a[k], b[k]), k
    for x, y in zip(a["stats"], b["stats"]):
        assert torch.equal(x, y)
    for x, y in zip(ra, rb):
        assert x["n/ep"] == y["n/ep"] and x["n/st"] == y["n/st"]
        assert np.array_equal(x["rews"], y["rews"]) and np.array_equal(x["lens"], y["lens"])
        assert np.array_equal(x["idxs"], y["idxs"])
    assert a["rms"][2] == b["rms"][2]
    np.testing.assert_allclose(a["rms"][0].numpy(), b["rms"][0].numpy(), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(a["rms"][1].numpy(), b["rms"][1].numpy(), rtol=1e-6, atol=1e-7)
    for k in ("obs", "obs_next", "cur"):
        np.testing.assert_allclose(a[k].numpy(), b[k].numpy(), rtol=1e-6, atol=1e-6, err_msg=k)
    np.testing.assert_allclose(a["act"].numpy(), b["act"].numpy(), rtol=1e-5, atol=1e-5)


def _assert_matches_four_launch_coupled(a, ra, b, rb):
    """test_fused_step_action_coupled_env's asserts."""
    for k in ("rew", "terminated", "truncated", "done", "env_id"):
        assert torch.equal(a[k], b[k]), k
    for x, y in zip(a["stats"], b["stats"]):
        assert torch.equal(x, y)
    for x, y in zip(ra, rb):
        assert x["n/ep"] == y["n/ep"] and np.array_equal(x["lens"], y["lens"])
        assert np.array_equal(x["rews"], y["rews"])
    assert a["rms"][2] == b["rms"][2]
    np.testing.assert_allclose(a["rms"][0].numpy(), b["rms"][0].numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(a["rms"][1].numpy(), b["rms"][1].numpy(), rtol=1e-5, atol=1e-6)
    for k in ("obs", "obs_next", "cur"):
        np.testing.assert_allclose(a[k].numpy(), b[k].numpy(), rtol=1e-5, atol=1e-5, err_msg=k)
    np.testing.assert_allclose(a["act"].numpy(), b["act"].numpy(), rtol=1e-5, atol=1e-5)


def _check(dev, E, D, L, T, G, collects=1):
    """The default env: fused (graph_steps G) against the four-launch step, against a second
    fused run, and fused graph_steps 0 against 4."""
    A = 17 if D >= 17 else 2
    runs = {}

    def fused(g):
        if g not in runs:
            runs[g] = _run(dev, True, E, D, A, L, T, g, collects)
        return runs[g]

    a, ra = fused(G)
    b, rb = _run(dev, False, E, D, A, L, T, G, collects)
    _assert_matches_four_launch(a, ra, b, rb)
    a2, ra2 = _run(dev, True, E, D, A, L, T, G, collects)
    _assert_bit_equal(a, ra, a2, ra2, "two fused runs")
    g0, r0 = fused(0)
    g4, r4 = fused(4)
    _assert_bit_equal(g0, r0, g4, r4, "graph_steps 0 vs 4")


@pytest.mark.parametrize("D", [5, 17, 376, 496, 500, 512])
def test_column_count_against_thread_split(dev, D):
    """D = 5, 17: almost every thread spare, D % 4 != 0; 376: 136 spare threads; 496 = NT - R:
    exactly the key threads spare; 500, 512: no spare threads, one thread per column."""
    _check(dev, 33, D, 3, 7, 4)


@pytest.mark.parametrize("E", [7, 100, 33])
def test_partial_row_tiles(dev, E):
    """One workgroup of 7 rows; a last workgroup of 4 rows; one extra row."""
    _check(dev, E, 376, 5, 7, 4)


@pytest.mark.parametrize("L", [1, 2, 3])
def test_resets_in_every_step(dev, L):
    """Every reset-row hash, and reset rows in every launch."""
    _check(dev, 100, 376, L, 7, 4)


@pytest.mark.parametrize("G", [0, 2, 4, 6])
def test_chain_structure(dev, G):
    """T = 7: the first launch without a merge, the totals ring wrapping, a remainder graph,
    the closing plain add.  The collector captures graphs of an even number of steps only
    (Collector._replay_steps asserts it: the step counters ping-pong), so the odd
    graph_steps 1 and 3 cannot run; their nearest even values stand in: 2 (three graphs of
    two steps), 4 (one graph and a remainder graph of two) and 6 (the chain's six graphed
    steps as one graph), next to 0 (eager launches only)."""
    _check(dev, 100, 376, 3, 7, G)


def test_two_collects_on_one_collector(dev):
    """The state carried between collects."""
    _check(dev, 100, 376, 3, 7, 4, collects=2)


@pytest.mark.parametrize("E,D,A", [(100, 376, 17), (33, 17, 6)])
def test_action_coupled_env(dev, E, D, A):
    """act_coef = 0.05: coupled_val's hash half needs no action, its final add does.  (This
    env's obs_rms moments are f64 atomic sums, so no bit-equality between runs is asserted
    here.)"""
    a, ra = _run(dev, True, E, D, A, 3, 7, 4, act_coef=0.05)
    b, rb = _run(dev, False, E, D, A, 3, 7, 4, act_coef=0.05)
    _assert_matches_four_launch_coupled(a, ra, b, rb)
