"""tests/golden/ddpg.npz (tools/gen_goldens.py gen_ddpg) pinned on the host, and the host parts
of DDPGPolicy / TD3Policy: the noise processes of tianshou_amd.exploration bit for bit, the
``Actor`` head, the constructor assertions, and a plain-torch restatement of ddpg.py:168-194,
td3.py:98-134 and the soft update (written here, no tianshou_amd policy involved) that replays
every recorded variant from the recorded indices and torch.randn draws.

Tolerances of the replay (the ones tests/test_gpu_ddpg.py holds the device path to): returns
rtol 1e-5, critic losses rtol 2e-5, actor loss within 2e-5 * mean|Q| of the recorded critic
outputs (a signed mean), outgoing weights rtol 1e-4, parameters rtol 1e-5 / atol 1e-6."""
from copy import deepcopy

import numpy as np
import pytest
import torch

from tests import ddpg_common as common


@pytest.fixture(scope="module")
def z(golden_dir):
    return common.golden(golden_dir)


# -- (a) noise processes ----------------------------------------------------------------------------
def test_noise_cases_cover_the_issue(z):
    cases = common.noise_cases(z)
    assert [(c["k"], c["A"]) for c in cases[::4]] == [(1, 1), (65, 6), (257, 17)]
    assert [(c["kind"], c["kw"], c["calls"]) for c in cases[:4]] == [
        ("none", {}, 1), ("gauss", {"sigma": 0.1}, 1), ("gauss", {"mu": 0.05, "sigma": 0.3}, 1),
        ("ou", {}, 3)]


def test_noise_processes_reproduce_reference(z):
    for i, c in enumerate(common.noise_cases(z)):
        if c["kind"] == "none":
            continue
        p = f"noise{i}_"
        noise = common.make_noise(c)
        act = z[p + "act_in"]
        assert act.dtype == np.float32 and act.shape == (c["k"], c["A"])
        np.random.seed(c["seed"])
        for call in range(c["calls"]):
            out = act + noise(act.shape)
            assert out.dtype == np.float64
            np.testing.assert_array_equal(out, z[p + "act_out"][call], err_msg=f"{p}{call}")
        common.assert_np_state(z, p)
        if c["kind"] == "ou":
            np.testing.assert_array_equal(noise._x, z[p + "ou_x"])
            # a changed shape restarts the process from 0
            np.random.seed(1)
            first = noise((2, 2))
            np.random.seed(1)
            assert np.array_equal(first, noise._beta * np.random.normal(size=(2, 2)))
            # reset(): back to x0 (None), so the recorded first call comes out again
            noise.reset()
            assert noise._x is None
            np.random.seed(c["seed"])
            np.testing.assert_array_equal(act + noise(act.shape), z[p + "act_out"][0])


def test_noise_defaults_and_assertion():
    from tianshou_amd.exploration import BaseNoise, GaussianNoise, OUNoise
    g = GaussianNoise()
    assert (g._mu, g._sigma) == (0.0, 1.0) and isinstance(g, BaseNoise)
    with pytest.raises(AssertionError, match="Noise std should not be negative"):
        GaussianNoise(sigma=-0.1)
    ou = OUNoise()
    assert ou._mu == 0.0 and ou._alpha == 0.15 * 1e-2 and ou._beta == 0.3 * np.sqrt(1e-2)
    assert ou._x is None
    ou5 = OUNoise(x0=0.5)
    np.random.seed(0)
    r = ou5._beta * np.random.normal(size=(3,))
    np.random.seed(0)
    assert np.array_equal(ou5((3,)), 0.5 + ou5._alpha * (0.0 - 0.5) + r)
    with pytest.raises(TypeError):
        BaseNoise()


def test_policy_noise_on_numpy_actions(z):
    from tianshou_amd.data import Batch
    from tianshou_amd.policy import DDPGPolicy
    for i, c in enumerate(common.noise_cases(z)):
        p = f"noise{i}_"
        policy = DDPGPolicy(None, None, None, None, exploration_noise=common.make_noise(c),
                            action_scaling=False)
        act = z[p + "act_in"]
        np.random.seed(c["seed"])
        for call in range(c["calls"]):
            out = policy.exploration_noise(act, Batch())
            if c["kind"] == "none":
                assert out is act
            else:
                np.testing.assert_array_equal(out, z[p + "act_out"][call])
        common.assert_np_state(z, p)
    policy.set_exp_noise(None)
    assert policy.exploration_noise(act, Batch()) is act


# -- nets and constructors ----------------------------------------------------------------------------
def test_actor_matches_recorded_forward(z):
    cfg = common.learn_cfg(z)
    actor = common.make_nets(z, cfg, "ddpg", "cpu")["actor"]
    assert [k for k, _ in actor.named_parameters()] == [
        k[len("ddpg_init_actor."):] for k in z if k.startswith("ddpg_init_actor.")]
    assert set(actor.state_dict()) >= {"preprocess.model.model.0.weight",
                                       "preprocess_net.model.model.0.weight",
                                       "last.model.0.weight"}
    with torch.no_grad():
        act, hidden = actor(z["actor_fwd_obs"], state="s")
    assert hidden == "s" and act.shape == (len(z["actor_fwd_obs"]), cfg["A"])
    np.testing.assert_allclose(act.numpy(), z["actor_fwd_act"], rtol=1e-6, atol=1e-7)
    assert float(act.abs().max()) < 1.0
    actor.max_action = 2.5
    with torch.no_grad():
        np.testing.assert_allclose(actor(z["actor_fwd_obs"])[0].numpy(),
                                   2.5 * z["actor_fwd_act"], rtol=1e-6, atol=1e-7)


def test_constructor_assertions(z):
    from tianshou_amd.policy import DDPGPolicy, TD3Policy
    cfg = common.learn_cfg(z)
    nets = common.make_nets(z, cfg, "td3", "cpu")
    opt = {n: common.make_optim("adam", m.parameters()) for n, m in nets.items()}
    args = (nets["actor"], opt["actor"], nets["critic1"], opt["critic1"])
    td3_args = args + (nets["critic2"], opt["critic2"])
    for bad in (-0.1, 1.5):
        with pytest.raises(AssertionError, match="tau should be in"):
            DDPGPolicy(*args, tau=bad, action_scaling=False)
        with pytest.raises(AssertionError, match="gamma should be in"):
            TD3Policy(*td3_args, gamma=bad, action_scaling=False)
    with pytest.raises(AssertionError, match="tanh mapping is not supported"):
        DDPGPolicy(*args, action_scaling=False, action_bound_method="tanh")
    with pytest.raises(AssertionError, match="tanh mapping is not supported"):
        TD3Policy(*td3_args, action_scaling=False, action_bound_method="tanh")
    nets["actor"].max_action = 2.0
    from tianshou_amd.env import Box
    with pytest.warns(UserWarning, match="max_action=2.0"):
        DDPGPolicy(*args, action_space=Box(-1.0, 1.0, (cfg["A"],)))
    nets["actor"].max_action = 1.0
    p = TD3Policy(*td3_args, action_scaling=False)
    assert (p.tau, p._gamma, p._policy_noise, p._freq, p._noise_clip, p._cnt, p._last) == \
        (0.005, 0.99, 0.2, 2, 0.5, 0, 0)
    assert p._noise._sigma == 0.1 and p.fused and p.fused_adam and p.graph_learn is None
    assert not p.actor_old.training and not p.critic1_old.training
    assert p.train(False).critic2.training is False and p.train().actor.training
    assert not p.critic2_old.training and not p.actor_old.training


# -- (b) plain-torch replay of every variant ------------------------------------------------------------
class HostRing:
    """The add() stream of ddpg.npz laid out as VectorReplayBuffer lays it out (E sub-rings of
    S rows), with the reference's n-step return (base.py:386-440, 500-524) restated in f64."""

    def __init__(self, z, cfg):
        E, S = cfg["E"], cfg["S"]
        self.S = S
        n = E * S
        self.obs = np.zeros((n, cfg["D"]), np.float32)
        self.obs_next = np.zeros((n, cfg["D"]), np.float32)
        self.act = np.zeros((n, cfg["A"]), np.float32)
        self.rew = np.zeros(n, np.float64)
        self.term = np.zeros(n, bool)
        self.done = np.zeros(n, bool)
        ptr, self.last = [0] * E, [0] * E
        for r, e in enumerate(z["add_ids"]):
            i = e * S + ptr[e]
            self.obs[i], self.obs_next[i], self.act[i] = \
                z["add_obs"][r], z["add_obs_next"][r], z["add_act"][r]
            self.rew[i], self.term[i] = z["add_rew"][r], z["add_terminated"][r]
            self.done[i] = z["add_terminated"][r] or z["add_truncated"][r]
            self.last[e], ptr[e] = i, (ptr[e] + 1) % S
        assert self.last == z["buf_last_index"].tolist()

    def ends(self, i):
        return bool(self.done[i]) or i == self.last[i // self.S]

    def nstep(self, indices, target_q_fn, gamma, n_step):
        """(returns [b] f32) with target_q_fn(terminal rows) -> [b] f32."""
        terminal, partial, power = [], [], []
        for i in indices.tolist():
            ret, g = 0.0, 1.0
            for k in range(n_step):
                ret += g * self.rew[i]
                g *= gamma
                if self.ends(i) or k == n_step - 1:
                    break
                base = (i // self.S) * self.S
                i = base + (i - base + 1) % self.S
            terminal.append(i)
            partial.append(ret)
            power.append(g)
        terminal = np.array(terminal)
        tq = target_q_fn(terminal).astype(np.float64) * ~self.term[terminal]
        return (tq * np.array(power) + np.array(partial)).astype(np.float32)


def _mse_step(critic, optim, obs, act, returns, weight):
    q = critic(obs, act).flatten()
    td = q - returns
    loss = (td.pow(2) * weight).mean()
    optim.zero_grad()
    loss.backward()
    optim.step()
    return td.detach(), loss.item()


def _soft(tgt, src, tau):
    for tp, sp in zip(tgt.parameters(), src.parameters()):
        tp.data.copy_(tau * sp.data + (1 - tau) * tp.data)


class _Holder:
    pass


@pytest.mark.parametrize("tag", common.DDPG_TAGS + common.TD3_TAGS)
def test_plain_torch_replay_matches_recording(z, tag):
    cfg = common.learn_cfg(z)
    v = cfg["variants"][tag]
    kind, tau, gamma = v["kind"], cfg["tau"], cfg["gamma"]
    names = cfg["nets"][kind]
    critics = names[1:]
    ring = HostRing(z, cfg)
    h = _Holder()
    for n, m in common.make_nets(z, cfg, kind, "cpu").items():
        setattr(h, n, m)
        setattr(h, n + "_old", deepcopy(m))
    opt = {n: common.make_optim(v["optim"], getattr(h, n).parameters()) for n in names}
    cnt, last = 0, 0.0
    for u in range(common.N_UPDATES):
        idx = z[tag + "_indices"][u]
        assert len(idx) == v["bs"]

        def target_q(rows):
            with torch.no_grad():
                obs_next = torch.as_tensor(ring.obs_next[rows])
                a = h.actor_old(obs_next)[0]
                if kind == "ddpg":
                    return h.critic_old(obs_next, a).flatten().numpy()
                noise = torch.as_tensor(z[tag + "_randn"][u]) * v["policy_noise"]
                if v["noise_clip"] > 0.0:
                    noise = noise.clamp(-v["noise_clip"], v["noise_clip"])
                a += noise
                return torch.min(h.critic1_old(obs_next, a),
                                 h.critic2_old(obs_next, a)).flatten().numpy()

        returns = ring.nstep(idx, target_q, gamma, v["n_step"])
        np.testing.assert_allclose(returns, z[tag + "_returns"][u].reshape(-1), rtol=1e-5,
                                   err_msg=f"{tag} {u}")
        obs, act = torch.as_tensor(ring.obs[idx]), torch.as_tensor(ring.act[idx])
        weight = torch.as_tensor(z[tag + "_weight"][u]) if v.get("per") else 1.0
        ret_t = torch.as_tensor(returns)
        tds, losses = zip(*[_mse_step(getattr(h, c), opt[c], obs, act, ret_t, weight)
                            for c in critics])
        td = tds[0] if kind == "ddpg" else (tds[0] + tds[1]) / 2.0
        do_actor = kind == "ddpg" or cnt % v["freq"] == 0
        q_scale = float(np.abs(z[tag + "_q_obs"][u]).mean())
        if do_actor:
            actor_loss = -getattr(h, critics[0])(obs, h.actor(obs)[0]).mean()
            opt["actor"].zero_grad()
            actor_loss.backward()
            last = actor_loss.item()
            opt["actor"].step()
            for n in (names if kind == "ddpg" else critics + ["actor"]):
                _soft(getattr(h, n + "_old"), getattr(h, n), tau)
        cnt += 1
        for c, loss in zip(critics, losses):
            np.testing.assert_allclose(loss, float(z[f"{tag}_loss_{c}"][u]), rtol=2e-5)
        assert abs(last - float(z[tag + "_loss_actor"][u])) <= 2e-5 * q_scale
        if kind == "td3":
            assert cnt == int(z[tag + "_cnt"][u])
            assert abs(last - float(z[tag + "_last"][u])) <= 2e-5 * q_scale
        np.testing.assert_allclose(td.numpy(), z[tag + "_td"][u], rtol=1e-4)
        np.testing.assert_allclose(common.flat_params(h, names), z[tag + "_params"][u],
                                   rtol=1e-5, atol=1e-6, err_msg=f"{tag} update {u}")
    if kind == "td3":  # the schedule the variant was chosen for
        carried = [float(x) for x in z[tag + "_last"]]
        steps = [u for u in range(common.N_UPDATES) if u % v["freq"] == 0]
        assert all(carried[u] == carried[max(s for s in steps if s <= u)]
                   for u in range(common.N_UPDATES))
        assert len(set(carried)) == len(steps)


def test_recorded_variants_are_the_issue_table(z):
    cfg = common.learn_cfg(z)
    want = {
        "ddpg": dict(kind="ddpg", n_step=1, bs=64, optim="adam"),
        "ddpg_nstep": dict(kind="ddpg", n_step=3, bs=65, optim="adam"),
        "ddpg_per": dict(kind="ddpg", n_step=1, bs=32, optim="adam", per=True),
        "ddpg_rms": dict(kind="ddpg", n_step=1, bs=64, optim="rms"),
        "td3": dict(kind="td3", n_step=1, bs=64, optim="adam", freq=2, policy_noise=0.2,
                    noise_clip=0.5),
        "td3_noclip": dict(kind="td3", n_step=2, bs=65, optim="adam", freq=1, policy_noise=0.2,
                           noise_clip=0.0),
        "td3_per": dict(kind="td3", n_step=1, bs=32, optim="adam", freq=3, policy_noise=0.2,
                        noise_clip=0.5, per=True),
        "td3_nonoise": dict(kind="td3", n_step=1, bs=64, optim="adam", freq=2, policy_noise=0.0,
                            noise_clip=0.5),
    }
    assert cfg["variants"] == want
    assert (cfg["E"], cfg["S"], cfg["D"], cfg["A"], cfg["hidden"]) == (6, 40, 5, 3, [16, 16])
    assert z["add_act"].dtype == np.float32 and z["add_act"].shape[1] == 3
    assert np.abs(z["add_act"]).max() <= 1.0
    assert (z["buf_lengths"] == 40).sum() == 1  # one env wrapped its sub-ring
    # the clip of td3.py:103 binds on both sides in the recorded draws
    d = z["td3_randn"] * 0.2
    assert (d > 0.5).any() and (d < -0.5).any()
