"""tests/golden/sac.npz (tools/gen_goldens.py gen_sac) pinned on the host, and the host parts of
SACPolicy: the constructor assertions, train() / sync_weight semantics, the C ABI symbols, and
the torch leg (``forward``, ``_target_q`` and ``learn`` on the CPU) replaying every recorded
variant from the recorded indices and draws over tests/test_ddpg_host.py's HostRing.

Tolerances of the replay (the ones tests/test_gpu_sac.py holds the device path to): returns
rtol 1e-5 / atol 1e-6, critic losses rtol 2e-5, outgoing weights rtol 1e-4, parameters,
log_alpha and alpha rtol 1e-5 / atol 1e-6, actor and temperature losses by
sac_common.actor_loss_bound / alpha_loss_bound."""
import os
import re

import numpy as np
import pytest
import torch

from tests import sac_common as common
from tests.test_ddpg_host import HostRing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("tsrl_sac_sample_fwd", "tsrl_sac_sample_bwd", "tsrl_sac_target",
           "tsrl_sac_actor_loss_fwd_bwd")


@pytest.fixture(scope="module")
def z(golden_dir):
    return common.golden(golden_dir)


def test_c_abi_symbols_are_declared_and_bound():
    from tianshou_amd import _C
    with open(os.path.join(ROOT, "include", "tsrl.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert name in _C.EXPORTED
        assert re.search(r"\bint " + name + r"\(", header), name
        assert _C._SIGS[name][0][-1] is _C._p  # the stream comes last


def test_recorded_variants_are_the_issue_table(z):
    cfg = common.learn_cfg(z)
    assert cfg["variants"] == {
        "sac": dict(init="sac", auto=False, n_step=1, bs=64, optim="adam"),
        "sac_auto": dict(init="sac", auto=True, n_step=3, bs=65, optim="adam"),
        "sac_per": dict(init="sac", auto=True, n_step=1, bs=32, optim="adam", per=True),
        "sac_rms": dict(init="sac", auto=True, n_step=1, bs=64, optim="rms"),
        "sac_bounded": dict(init="sac_bounded", auto=False, n_step=1, bs=64, optim="adam",
                            bounded=True),
    }
    assert (cfg["E"], cfg["S"], cfg["D"], cfg["A"], cfg["hidden"]) == (6, 40, 5, 3, [16, 16])
    assert (cfg["alpha"], cfg["alpha_lr"], cfg["target_entropy"], cfg["tau"], cfg["gamma"]) == \
        (0.2, 3e-3, -3.0, 0.05, 0.97)
    for tag, v in cfg["variants"].items():
        for k in ("eps_target", "eps_learn"):
            d = z[f"{tag}_{k}"]
            assert d.shape == (common.N_UPDATES, v["bs"], 3) and d.dtype == np.float32
            assert np.abs(d).max() <= 2.0
        # the conditions gen_sac asserted on the reference
        assert np.abs(z[tag + "_q1a"].astype(np.float64) - z[tag + "_q2a"]).min() >= 1e-4
    assert (np.abs(z["sac_eps_learn"]) == 2.0).any()  # the recorder's clamp binds
    a = z["fwd_train_act"].astype(np.float64)
    assert (1.0 - a * a).min() >= 0.02


def _policy_args(z, dev="cpu"):
    cfg = common.learn_cfg(z)
    nets = common.make_nets(z, cfg, cfg["variants"]["sac"], dev)
    opt = {n: common.make_optim("adam", m.parameters()) for n, m in nets.items()}
    return cfg, nets, (nets["actor"], opt["actor"], nets["critic1"], opt["critic1"],
                       nets["critic2"], opt["critic2"])


def test_constructor_assertions_and_defaults(z):
    from tianshou_amd.policy import DDPGPolicy, SACPolicy
    cfg, nets, args = _policy_args(z)
    for bad in (-0.1, 1.5):
        with pytest.raises(AssertionError, match="tau should be in"):
            SACPolicy(*args, tau=bad, action_scaling=False)
        with pytest.raises(AssertionError, match="gamma should be in"):
            SACPolicy(*args, gamma=bad, action_scaling=False)
    with pytest.raises(AssertionError, match="tanh mapping is not supported"):
        SACPolicy(*args, action_scaling=False, action_bound_method="tanh")
    for log_alpha in (torch.zeros(2, requires_grad=True), torch.zeros(1),
                      torch.zeros((), requires_grad=True)):
        with pytest.raises(AssertionError):
            SACPolicy(*args, alpha=(-3.0, log_alpha, None), action_scaling=False)
    p = SACPolicy(*args, action_scaling=False)
    assert isinstance(p, DDPGPolicy)
    assert (p.tau, p._gamma, p._alpha, p._is_auto_alpha, p._n_step, p._rew_norm, p._noise,
            p._deterministic_eval) == (0.005, 0.99, 0.2, False, 1, False, None, True)
    assert p.fused and p.fused_adam and p.graph_learn is None
    assert not hasattr(p, "actor_old") and not hasattr(p, "critic")
    assert p._sync_order == ("critic1", "critic2")
    assert p._optim_order == ("critic1", "critic2", "actor")
    log_alpha = torch.full((1,), 0.5, requires_grad=True)
    optim = torch.optim.Adam([log_alpha], lr=3e-3)
    p = SACPolicy(*args, alpha=(-3.0, log_alpha, optim), action_scaling=False)
    assert p._is_auto_alpha and p._target_entropy == -3.0 and p._log_alpha is log_alpha
    assert p._alpha_optim is optim and not p._alpha.requires_grad
    assert torch.equal(p._alpha, log_alpha.detach().exp())


def test_ddpg_and_td3_keep_their_orders(z):
    from tianshou_amd.policy import DDPGPolicy, TD3Policy
    assert DDPGPolicy._sync_order == ("actor", "critic")
    assert TD3Policy._sync_order == ("critic1", "critic2", "actor")
    cfg, nets, args = _policy_args(z)
    assert DDPGPolicy(*args[:4], action_scaling=False)._optim_order == ("actor", "critic")
    assert TD3Policy(*args, action_scaling=False)._optim_order == \
        ("critic1", "critic2", "actor")


def test_train_and_sync_weight_semantics(z):
    from copy import deepcopy
    from tianshou_amd.policy import SACPolicy
    cfg, nets, args = _policy_args(z)
    p = SACPolicy(*args, tau=0.25, action_scaling=False)
    assert not p.critic1_old.training and not p.critic2_old.training
    assert p.train(False) is p and not p.training
    assert not (p.actor.training or p.critic1.training or p.critic2.training)
    assert p.train() is p and p.training
    assert p.actor.training and p.critic1.training and p.critic2.training
    assert not p.critic1_old.training and not p.critic2_old.training
    # sync_weight: the two critics only, tau * online + (1 - tau) * target
    with torch.no_grad():
        for net in (p.actor, p.critic1, p.critic2):
            for t in net.parameters():
                t.add_(0.5)
    before = {n: deepcopy(getattr(p, n + "_old")) for n in ("critic1", "critic2")}
    actor_before = [t.detach().clone() for t in p.actor.parameters()]
    p.sync_weight()
    for n in ("critic1", "critic2"):
        for t, s, o in zip(getattr(p, n + "_old").parameters(), getattr(p, n).parameters(),
                           before[n].parameters()):
            assert torch.equal(t, 0.25 * s + 0.75 * o) and not torch.equal(t, o)
    for t, o in zip(p.actor.parameters(), actor_before):
        assert torch.equal(t, o)


def test_forward_reproduces_recorded_forwards(z):
    from tianshou_amd.data import Batch
    cfg = common.learn_cfg(z)
    policy, _ = common.make_policy(z, cfg, "sac", "cpu")
    obs = z["fwd_obs"]
    for mode in ("eval", "train"):
        policy.train(mode == "train")
        common.feed_draws(policy, [z["fwd_train_eps"]] if mode == "train" else [])
        with torch.no_grad():
            res = policy(Batch(obs=obs, info=Batch()))
        assert set(res.keys()) == {"logits", "act", "state", "dist", "log_prob"}
        assert res.log_prob.shape == (len(obs), 1) and res.state is None
        np.testing.assert_allclose(res.logits[0].numpy(), z[f"fwd_{mode}_mu"], rtol=1e-6,
                                   atol=1e-7)
        np.testing.assert_allclose(res.logits[1].numpy(), z[f"fwd_{mode}_sigma"], rtol=1e-6)
        np.testing.assert_allclose(res.act.numpy(), z[f"fwd_{mode}_act"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(res.log_prob.numpy(), z[f"fwd_{mode}_log_prob"], rtol=1e-5)
        assert isinstance(res.dist, torch.distributions.Independent)
    policy.train(False)
    with torch.no_grad():
        res = policy(Batch(obs=obs, info=Batch()))
    assert torch.equal(res.act, torch.tanh(res.logits[0]))  # deterministic_eval
    policy._deterministic_eval = False
    common.feed_draws(policy, [z["fwd_train_eps"]])
    with torch.no_grad():
        res = policy(Batch(obs=obs, info=Batch()))
    np.testing.assert_allclose(res.act.numpy(), z["fwd_train_act"], rtol=1e-6, atol=1e-7)


class _ObsNext:
    """What DDPGPolicy._obs_next reads of a buffer."""

    def __init__(self, ring):
        self.ring = ring

    def get(self, indices, key):
        assert key == "obs_next"
        return torch.as_tensor(self.ring.obs_next[indices])


@pytest.mark.parametrize("tag", common.TAGS)
def test_torch_leg_replays_recording_on_cpu(z, tag):
    from tianshou_amd.data import Batch
    cfg = common.learn_cfg(z)
    policy, v = common.make_policy(z, cfg, tag, "cpu")
    policy.train()
    common.feed_draws(policy, common.update_draws(z, tag))
    ring = HostRing(z, cfg)
    stub = _ObsNext(ring)
    for u in range(common.N_UPDATES):
        q = f"{tag} update {u}"
        idx = z[tag + "_indices"][u]
        assert len(idx) == v["bs"]

        def target_q(rows):
            with torch.no_grad():
                return policy._target_q(stub, rows).flatten().numpy()

        returns = ring.nstep(idx, target_q, cfg["gamma"], v["n_step"])
        np.testing.assert_allclose(returns, z[tag + "_returns"][u].reshape(-1), rtol=1e-5,
                                   atol=1e-6, err_msg=q)
        batch = Batch(obs=torch.as_tensor(ring.obs[idx]), act=torch.as_tensor(ring.act[idx]),
                      returns=torch.as_tensor(returns), info=Batch())
        if v.get("per"):
            batch.weight = torch.as_tensor(z[tag + "_weight"][u])
        res = policy.learn(batch)
        assert set(res) == set(common.loss_keys(v["auto"]))
        for k in ("loss/critic1", "loss/critic2"):
            np.testing.assert_allclose(res[k], float(z[f"{tag}_{k.replace('/', '_')}"][u]),
                                       rtol=2e-5, err_msg=q)
        assert abs(res["loss/actor"] - float(z[tag + "_loss_actor"][u])) <= \
            common.actor_loss_bound(z, tag, u), q
        if v["auto"]:
            assert abs(res["loss/alpha"] - float(z[tag + "_loss_alpha"][u])) <= \
                common.alpha_loss_bound(z, cfg, tag, u), q
            np.testing.assert_allclose(res["alpha"], float(z[tag + "_alpha"][u]), rtol=1e-5,
                                       atol=1e-6, err_msg=q)
            np.testing.assert_allclose(policy._log_alpha.detach().numpy(),
                                       z[tag + "_log_alpha"][u], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(batch.weight.numpy(), z[tag + "_td"][u], rtol=1e-4,
                                   err_msg=q)
        np.testing.assert_allclose(common.flat_params(policy), z[tag + "_params"][u],
                                   rtol=1e-5, atol=1e-6, err_msg=q)
    with pytest.raises(StopIteration):  # exactly two draws per update
        policy._rsample_noise((1, 1), "cpu")
