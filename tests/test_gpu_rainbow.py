"""RainbowPolicy on the device path (tianshou_amd/policy/rainbow.py, utils/net.py NoisyLinear /
dueling Net, utils/net_atari.py Rainbow, csrc/noisy.hip).

update() against tests/golden/rainbow.npz (tools/gen_goldens.py gen_rainbow;
tests/test_rainbow_host.py pins that file) with the recorded noise injected in place of the
sampler.  Assertions and bounds are tests/test_gpu_dist_dqn.py's: sampled indices equal, returns
rtol 1e-5 / atol 1e-6, losses rtol 2e-5, outgoing weights rtol 1e-4, Adam parameters rtol 1e-5
/ atol 1e-6 (at the updates the file records them for), tree leaves, priorities and importance
weights rtol 1e-4.  With RMSprop the parameter bound is 4 x what ``fused = False`` (torch
autograd + torch.optim.RMSprop) deviates from the same recording in the same test.  Measured on
an MI355X, max |parameter - recorded|: RMSprop after updates 0 / 2 / 5 torch 3.35e-8 / 3.17e-8 /
2.98e-8, fused 6.33e-8 / 6.15e-8 / 5.96e-8; Adam at every recorded update fused 1.13e-6
("target"), 1.34e-7 ("per"), 2.09e-7 ("notarget"), torch 1.52e-6 ("target"), 4.02e-7 ("per");
losses equal to the recorded ones in 7 printed digits or one unit off, outgoing weights within
3.6e-7 relative, returns equal.  Atari: the largest gradient difference between the two legs
is 2.8e-9 (2.1e-7 of that tensor's largest gradient).

The Atari case compares one update of the fused path with ``fused = False`` from equal state and
noise: probabilities rtol 1e-5 / atol 1e-6 and rows summing to 1 within 1e-5 (test_atari_heads'
bound), loss rtol 2e-5, outgoing weights rtol 1e-4, and every gradient rtol 1e-4 with atol 1e-6
max|gradient| (the loss kernels' gradient bound); the parameters after Adam's first step are not
compared, because that step is lr * sign(g) wherever |g| >> 1e-8 and flips with the sign of a
gradient that is zero up to rounding."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from tianshou_amd.data import Batch
from tianshou_amd.policy import C51Policy, RainbowPolicy
from tianshou_amd.utils.net import NoisyLinear, noisy_layers, sample_noise

from tests import test_gpu_dqn as gd
from tests.test_rainbow_host import EPS_KEYS, init_state, inject_noise, make_net

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "rainbow.npz"))


def _cfg(z):
    return json.loads(str(z["learn_cfg"]))


def _policy(z, cfg, tag, dev, optim=None, **attrs):
    v = cfg["variants"][tag]
    net = make_net(cfg, dev).to(dev)
    net.load_state_dict(init_state(z))
    if optim is None:
        optim = v["optim"]
    opt = {"rms": lambda p: torch.optim.RMSprop(p, lr=7e-4, eps=1e-5, alpha=0.99),
           "adam": lambda p: torch.optim.Adam(p, lr=1e-3),
           "sgd": lambda p: torch.optim.SGD(p, lr=1e-2)}[optim](net.parameters())
    policy = RainbowPolicy(net, opt, **cfg["c51"], discount_factor=cfg["gamma"],
                           estimation_step=v["n_step"], target_update_freq=v["freq"]).to(dev)
    for k, a in attrs.items():
        setattr(policy, k, a)
    policy.train()
    return policy, v


def _param_dev(module, z, prefix):
    return max(float(np.abs(t.detach().cpu().numpy().astype(np.float64) - z[prefix + k]).max())
               for k, t in module.state_dict().items() if ".eps_" not in k)


def _run_variant(z, dev, tag, check_params, monkeypatch, **attrs):
    """Six update() calls of one recorded variant under the recorded noise; everything but the
    parameters is asserted here, the parameters by ``check_params(u, policy)`` at the updates
    the file has them for."""
    cfg = _cfg(z)
    policy, v = _policy(z, cfg, tag, dev, **attrs)
    buf = gd._filled_buffer(z, cfg, dev, per=bool(v.get("per")))
    step = [0, tag]
    inject_noise(monkeypatch, z, policy, step)
    seen = gd._record(policy)
    np.random.seed(cfg["seed"])
    for u in range(6):
        step[0] = u
        res = policy.update(v["bs"], buf)
        q = f"{tag}_u{u}_"
        s = seen[u]
        assert s["indices"].tolist() == z[q + "indices"].tolist(), q
        out_w = s["td_error"]  # the recorder's name for the outgoing batch.weight
        print(f"{q} loss {res['loss']:.7g} recorded {float(z[q + 'loss']):.7g} max rel dweight "
              f"{np.abs(out_w.cpu().numpy() / z[q + 'out_weight'] - 1).max():.3g} max|dreturns| "
              f"{np.abs(s['returns'].cpu().numpy() - z[q + 'returns']).max():.3g}")
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
        if v["freq"]:
            assert policy.model_old.training
            synced = u % v["freq"] == 0
            old, new = policy.model_old.state_dict(), policy.model.state_dict()
            for k in EPS_KEYS:  # a sync hands the online noise to the target
                assert torch.equal(old[k], new[k]) == synced, (q, k)
                assert torch.equal(new[k].cpu(), torch.as_tensor(z[f"{q}eps_model_{k}"]))
            if synced and u and (u - 1) in cfg["param_updates"][tag]:
                # the target holds the parameters recorded one update earlier
                for k, t in old.items():
                    if ".eps_" not in k:
                        np.testing.assert_allclose(
                            t.cpu().numpy(), z[f"{tag}_u{u - 1}_param_{k}"], rtol=1e-5,
                            atol=1e-6, err_msg=f"model_old {q}{k}")
        if u in cfg["param_updates"][tag]:
            print(f"{q} max|dparam| {_param_dev(policy.model, z, q + 'param_'):.3g}")
            check_params(u, policy)
    if v.get("per"):
        np.testing.assert_allclose(buf._max_prio, float(z[tag + "_max_prio"]), rtol=1e-4)
        np.testing.assert_allclose(buf._min_prio, float(z[tag + "_min_prio"]), rtol=1e-4)
    assert policy._iter == 6
    return policy


def _adam_check(z, tag):
    def check(u, policy):
        for k, t in policy.model.state_dict().items():
            if ".eps_" not in k:
                np.testing.assert_allclose(t.cpu().numpy(), z[f"{tag}_u{u}_param_{k}"],
                                           rtol=1e-5, atol=1e-6, err_msg=f"{tag} update {u} {k}")
    return check


@pytest.mark.parametrize("tag", ("target", "per", "notarget"))
def test_update_matches_reference_adam(z, dev, tag, monkeypatch):
    policy = _run_variant(z, dev, tag, _adam_check(z, tag), monkeypatch)
    assert policy._flat is not None and policy._flat.adam_bound(policy.optim)
    assert policy._learn_graphs and not policy._graph_failed  # these updates replay
    assert all(m.fused for m in noisy_layers(policy.model))


def test_update_matches_reference_rmsprop(z, dev, monkeypatch):
    """The fused path's max |parameter - recorded| at each recorded update stays within 4 x the
    torch formulation's on the same GPU (both printed)."""
    torch_dev, fused_dev = {}, {}
    _run_variant(z, dev, "rms", lambda u, p: torch_dev.__setitem__(
        u, _param_dev(p.model, z, f"rms_u{u}_param_")), monkeypatch, fused=False)
    policy = _run_variant(z, dev, "rms", lambda u, p: fused_dev.__setitem__(
        u, _param_dev(p.model, z, f"rms_u{u}_param_")), monkeypatch)
    print("rms max|dparam| per recorded update: torch", torch_dev, "fused", fused_dev)
    assert policy._flat.adam_bound(policy.optim)
    assert set(policy.optim.state[next(policy.model.parameters())]) == {"step", "square_avg"}
    assert sorted(fused_dev) == _cfg(z)["param_updates"]["rms"]
    for u in fused_dev:
        assert fused_dev[u] <= 4 * torch_dev[u], (u, fused_dev[u], torch_dev[u])


@pytest.mark.parametrize("tag", ("target", "per"))
def test_torch_formulation_matches_reference(z, dev, tag, monkeypatch):
    policy = _run_variant(z, dev, tag, _adam_check(z, tag), monkeypatch, fused=False)
    assert policy._flat is None and not policy._learn_graphs
    assert not any(m.fused for m in noisy_layers(policy.model, policy.model_old))


# -- the sampler and the graph ---------------------------------------------------------------------
def _six_updates(z, dev, tag, seed, **attrs):
    """Six updates with fresh sampled noise each (the device generator seeded)."""
    cfg = _cfg(z)
    policy, v = _policy(z, cfg, tag, dev, **attrs)
    buf = gd._filled_buffer(z, cfg, dev, per=bool(v.get("per")))
    np.random.seed(cfg["seed"])
    torch.manual_seed(seed)
    out = []
    for _ in range(6):
        loss = policy.update(v["bs"], buf)["loss"]
        out.append((loss, [t.detach().clone() for t in policy.model.state_dict().values()],
                    [t.detach().clone() for t in policy.model_old.state_dict().values()]
                    if v["freq"] else []))
    return policy, out


@pytest.mark.parametrize("tag", ("target", "per", "notarget"))
def test_graph_replay_is_bitwise_eager(z, dev, tag):
    pol_g, out_g = _six_updates(z, dev, tag, 9, graph_learn=True)
    pol_e, out_e = _six_updates(z, dev, tag, 9, graph_learn=False)
    assert len(pol_g._learn_graphs) == 1 and not pol_e._learn_graphs
    eps = []
    for (loss_g, sd_g, old_g), (loss_e, sd_e, old_e) in zip(out_g, out_e):
        assert loss_g == loss_e
        for a, b in zip(sd_g + old_g, sd_e + old_e):
            assert torch.equal(a, b)
        eps.append(sd_g[list(pol_g.model.state_dict()).index(EPS_KEYS[0])])
    assert all(not torch.equal(eps[i], eps[i + 1]) for i in range(5))  # fresh noise each


def test_seeded_sampling_is_torch_randn_and_f(z, dev):
    cfg = _cfg(z)
    net = make_net(cfg, dev).to(dev)
    ptrs = None
    runs = []
    for _ in range(2):
        torch.manual_seed(31)
        assert sample_noise(net) is True
        runs.append([m.eps_p.clone() for m in noisy_layers(net)] +
                    [m.eps_q.clone() for m in noisy_layers(net)])
        now = [t.data_ptr() for m in noisy_layers(net) for t in (m.eps_p, m.eps_q)]
        assert ptrs is None or ptrs == now  # the buffers keep their addresses
        ptrs = now
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    torch.manual_seed(31)
    for m in noisy_layers(net):  # the reference's calls in the reference's order
        xp = torch.randn(m.in_features, device=dev)
        xq = torch.randn(m.out_features, device=dev)
        assert torch.equal(m.eps_p, xp.sign().mul_(xp.abs().sqrt_()))
        assert torch.equal(m.eps_q, xq.sign().mul_(xq.abs().sqrt_()))
    assert set(net.state_dict()) == set(init_state(z))
    assert sample_noise(torch.nn.Linear(2, 2).to(dev)) is False
    # fused = False: the reference's per-layer sample(), the same values
    for m in noisy_layers(net):
        m.fused = False
    torch.manual_seed(31)
    sample_noise(net)
    assert all(torch.equal(a, b) for a, b in
               zip(runs[0], [m.eps_p for m in noisy_layers(net)] +
                   [m.eps_q for m in noisy_layers(net)]))


# -- cache freshness -------------------------------------------------------------------------------
def _reference_forward(net, obs):
    """common.py:273-284 over discrete.py:369-379 on the current tensors, all torch."""
    def noisy(m, x):
        w = m.mu_W + m.sigma_W * m.eps_q.ger(m.eps_p)
        b = m.mu_bias + m.sigma_bias * m.eps_q.clone()
        return torch.nn.functional.linear(x, w, b)

    def head(mlp, x):
        return noisy(mlp.model[2], torch.relu(noisy(mlp.model[0], x)))

    with torch.no_grad():
        h = net.model(obs)
        q, v = head(net.Q, h).view(len(obs), -1, 51), head(net.V, h).view(len(obs), -1, 51)
        return torch.softmax(q - q.mean(dim=1, keepdim=True) + v, dim=-1)


def _assert_fresh(net, obs, what):
    assert net.training
    with torch.no_grad():
        got, _ = net(obs)
    torch.testing.assert_close(got, _reference_forward(net, obs), rtol=1e-5, atol=1e-6,
                               msg=lambda m: f"stale after {what}: {m}")
    for m in noisy_layers(net):  # and the cached parameters are the reference's bits
        assert torch.equal(m._W_eff, m.mu_W + m.sigma_W * m.eps_q.ger(m.eps_p)), what
        assert torch.equal(m._b_eff, m.mu_bias + m.sigma_bias * m.eps_q), what


@pytest.mark.parametrize("graph", (True, False))
def test_training_forward_is_never_stale(z, dev, graph):
    cfg = _cfg(z)
    policy, v = _policy(z, cfg, "target", dev, graph_learn=graph)
    buf = gd._filled_buffer(z, cfg, dev)
    obs = torch.randn(9, cfg["D"], generator=torch.Generator().manual_seed(1)).to(dev)
    net = policy.model
    _assert_fresh(net, obs, "construction")
    np.random.seed(2)
    torch.manual_seed(2)
    for u in range(4):
        policy.update(v["bs"], buf)
        _assert_fresh(net, obs, f"learn {u}")
        _assert_fresh(policy.model_old, obs, f"learn {u} (target)")
    assert bool(policy._learn_graphs) == graph
    policy.sync_weight()
    _assert_fresh(policy.model_old, obs, "sync_weight")
    for a, b in zip(policy.model_old.state_dict().values(), net.state_dict().values()):
        assert torch.equal(a, b)
    net.load_state_dict(init_state(z))
    _assert_fresh(net, obs, "load_state_dict")
    net.Q.model[2].sample()
    _assert_fresh(net, obs, "layer.sample()")
    net.V.model[0].sigma_W.data.mul_(1.5)
    net.Q.model[0].mu_bias.data.add_(0.25)
    _assert_fresh(net, obs, "p.data.mul_")
    twin = copy.deepcopy(net)
    twin.Q.model[0].mu_W.data.mul_(2.0)
    _assert_fresh(twin, obs, "deepcopy")
    _assert_fresh(net, obs, "deepcopy (the original)")
    for a, b in zip(noisy_layers(twin), noisy_layers(net)):
        assert a._W_eff.data_ptr() != b._W_eff.data_ptr()
    assert "_W_eff" not in "".join(net.state_dict())
    # eval-mode acting uses mu
    policy.eval()
    with torch.no_grad():
        act = policy(Batch(obs=obs, info=Batch())).act
        h = net.model(obs)
        mu = lambda m, x: torch.nn.functional.linear(x, m.mu_W, m.mu_bias)  # noqa: E731
        q = mu(net.Q.model[2], torch.relu(mu(net.Q.model[0], h))).view(9, -1, 51)
        val = mu(net.V.model[2], torch.relu(mu(net.V.model[0], h))).view(9, -1, 51)
        p = torch.softmax(q - q.mean(1, keepdim=True) + val, -1)
        torch.testing.assert_close(net(obs)[0], p, rtol=1e-5, atol=1e-6)
        out64 = net(obs)[0].double()
    assert torch.equal(act, (out64 * policy.support.double()).sum(2).argmax(1))
    policy.train()


# -- paths taken -----------------------------------------------------------------------------------
def test_flat_storage_is_bound_with_plain_adam(z, dev):
    cfg = _cfg(z)
    policy, v = _policy(z, cfg, "target", dev)
    buf = gd._filled_buffer(z, cfg, dev)
    np.random.seed(3)
    policy.update(v["bs"], buf)
    fa = policy._flat
    assert fa is not None and fa.adam_bound(policy.optim)
    flat = fa.flat_param
    lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * 4
    for p in policy.model.parameters():
        assert lo <= p.data_ptr() < hi
    for m in noisy_layers(policy.model):  # noise and effective parameters live elsewhere
        for t in (m.eps_p, m.eps_q, m._W_eff, m._b_eff):
            assert not lo <= t.data_ptr() < hi
    old = policy._old_flat
    assert old is not None and old.shape == flat.shape
    policy.update(v["bs"], buf)
    assert not torch.equal(old, flat)
    policy.sync_weight()
    assert torch.equal(old, flat)
    for a, b in zip(noisy_layers(policy.model_old), noisy_layers(policy.model)):
        assert torch.equal(a.eps_p, b.eps_p) and torch.equal(a.eps_q, b.eps_q)
        assert a.eps_p.data_ptr() != b.eps_p.data_ptr()


def test_other_optimisers_keep_torch_step(z, dev):
    cfg = _cfg(z)
    policy, v = _policy(z, cfg, "target", dev, optim="sgd")
    buf = gd._filled_buffer(z, cfg, dev)
    before = [p.detach().clone() for p in policy.model.parameters()]
    np.random.seed(3)
    losses = [policy.update(v["bs"], buf)["loss"] for _ in range(3)]
    assert policy._flat is None or not policy._flat.adam_bound(policy.optim)
    assert not policy._learn_graphs
    assert all(np.isfinite(losses)) and len(set(losses)) == 3
    assert all(not torch.equal(a, b) for a, b in zip(before, policy.model.parameters()))


def test_collect_greedy_fills_the_buffer(z, dev):
    """eps 0 in eval mode: the stored actions are the argmax of the torch-formulation Q-values
    of the mu network on the stored observations."""
    from tianshou_amd.data import Collector, VectorReplayBuffer
    from tianshou_amd.env import CartPoleEnv, Discrete, DummyVectorEnv
    from tianshou_amd.utils.net import Net
    E, n_step, size = 4, 80, 400
    envs = DummyVectorEnv([CartPoleEnv for _ in range(E)])
    np.random.seed(1627)
    torch.manual_seed(1627)
    envs.seed(1627)
    head = {"hidden_sizes": (16,), "linear_layer": lambda x, y: NoisyLinear(x, y, 0.5)}
    net = Net(4, 2, hidden_sizes=(16,), device=dev, softmax=True, num_atoms=51,
              dueling_param=(dict(head), dict(head))).to(dev)
    policy = RainbowPolicy(net, torch.optim.Adam(net.parameters(), lr=1e-3),
                           target_update_freq=10, action_space=Discrete(2)).to(dev)
    assert isinstance(policy, C51Policy)
    policy.set_eps(0.0)
    policy.eval()
    buf = VectorReplayBuffer(size, E, device=dev)
    res = Collector(policy, envs, buf, exploration_noise=True).collect(n_step=n_step)
    assert res["n/st"] == n_step and len(buf) == n_step
    steps, S = n_step // E, size // E
    m = buf._meta
    policy.fused = False
    with torch.no_grad():
        for t in range(steps):
            rows = torch.arange(E, device=dev) * S + t
            logits, _ = policy.model(m.obs[rows])
            assert logits.shape == (E, 2, 51)
            q = policy.compute_q_value(logits, None)
            assert torch.equal(m.act[rows].reshape(-1), q.argmax(dim=1)), t
    policy.fused = True
    policy.train()
    np.random.seed(4)
    losses = [policy.update(64, buf)["loss"] for _ in range(3)]
    assert all(np.isfinite(losses)) and len(set(losses)) == 3


# -- Atari -----------------------------------------------------------------------------------------
def test_atari_rainbow_update_matches_torch_formulation(dev):
    from tianshou_amd.utils.net_atari import DQN, Rainbow
    g = torch.Generator().manual_seed(2)
    b, A = 4, 6
    obs = torch.randint(0, 256, (b, 4, 84, 84), generator=g, dtype=torch.uint8).to(dev)
    obs_next = torch.randint(0, 256, (b, 4, 84, 84), generator=g, dtype=torch.uint8).to(dev)
    act = torch.randint(0, A, (b,), generator=g).to(dev)
    rew = torch.randn(b, 1, generator=g).to(dev)
    torch.manual_seed(0)
    net = Rainbow(4, 84, 84, [A], num_atoms=51, device=dev).to(dev)
    runs = []
    for fused in (True, False):
        twin = copy.deepcopy(net)
        policy = RainbowPolicy(twin, torch.optim.Adam(twin.parameters(), lr=1e-4),
                               target_update_freq=1).to(dev)
        policy.fused = fused
        policy.graph_learn = False
        policy.train()
        with torch.no_grad():
            probs, _ = twin(obs)
            feat, _ = DQN.forward(twin, obs)
        assert probs.shape == (b, A, 51) and feat.shape == (b, 3136)
        torch.testing.assert_close(probs.sum(-1), torch.ones(b, A, device=dev), rtol=0,
                                   atol=1e-5)
        batch = Batch(obs=obs, act=act, obs_next=obs_next, info=Batch(),
                      returns=rew + 0.99 * policy.support.detach().view(1, -1))
        torch.manual_seed(7)  # equal noise: both legs make the reference's draws
        loss = policy.learn(batch)["loss"]
        grads = {n: p.grad.detach().clone() for n, p in twin.named_parameters()}
        assert all(torch.isfinite(x).all() for x in grads.values())
        assert not any(torch.equal(p, q) for p, q in zip(twin.parameters(), net.parameters()))
        runs.append((probs, loss, batch.weight.clone(), grads,
                     [m.eps_q.clone() for m in noisy_layers(twin)]))
        assert (policy._flat is not None) == fused
    (p_f, loss_f, w_f, g_f, e_f), (p_t, loss_t, w_t, g_t, e_t) = runs
    assert all(torch.equal(a, c) for a, c in zip(e_f, e_t))
    torch.testing.assert_close(p_f, p_t, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(loss_f, loss_t, rtol=2e-5)
    torch.testing.assert_close(w_f, w_t, rtol=1e-4, atol=0)
    for n in g_f:
        scale = float(g_t[n].abs().max())
        err = float((g_f[n] - g_t[n]).abs().max())
        print(f"{n}: max|dgrad| {err:.3g} of max|grad| {scale:.3g}")
        torch.testing.assert_close(g_f[n], g_t[n], rtol=1e-4, atol=1e-6 * scale,
                                   msg=lambda m: f"{n}: {m}")
