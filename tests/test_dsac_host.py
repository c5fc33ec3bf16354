"""tests/golden/dsac.npz (tools/gen_goldens.py gen_dsac) pinned on the host, and the host parts
of DiscreteSACPolicy: constructor defaults, train() / sync_weight, exploration_noise, forward's
action modes, the C ABI symbols, the torch leg (``_target_q`` and ``learn`` on the CPU)
replaying every recorded variant from the recorded indices over tests/test_ddpg_host.py's
HostRing, and the f64 NumPy restatement of the kernels' formulas (tests/dsac_common.py)
against torch autograd in f64.

Tolerances of the replay are tests/test_sac_host.py's: returns rtol 1e-5 / atol 1e-6, critic
losses rtol 2e-5, outgoing weights rtol 1e-4, parameters, log_alpha and alpha rtol 1e-5 / atol
1e-6, actor and temperature losses by dsac_common.actor_loss_bound / alpha_loss_bound."""
import os
import re

import numpy as np
import pytest
import torch
from torch.distributions import Categorical

from tests import dsac_common as common
from tests.test_ddpg_host import HostRing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("tsrl_dsac_target", "tsrl_dsac_q_loss_fwd_bwd", "tsrl_dsac_actor_loss_fwd_bwd")


@pytest.fixture(scope="module")
def z(golden_dir):
    return common.golden(golden_dir)


def test_c_abi_symbols_are_declared_bound_and_exported():
    from tianshou_amd import _C
    with open(os.path.join(ROOT, "include", "tsrl.h")) as f:
        header = f.read()
    L = _C.lib()
    for name in SYMBOLS:
        assert name in _C.EXPORTED
        assert re.search(r"\bint " + name + r"\(", header), name
        assert _C._SIGS[name][0][-1] is _C._p  # the stream comes last
        assert getattr(L, name) is not None  # exported by the built library


def test_recorded_variants_are_the_issue_table(z):
    cfg = common.learn_cfg(z)
    assert cfg["variants"] == {
        "dsac": dict(auto=False, n_step=1, bs=64, optim="adam", seed=101),
        "dsac_auto": dict(auto=True, n_step=3, bs=65, optim="adam", seed=14),
        "dsac_per": dict(auto=True, n_step=1, bs=32, optim="adam", per=True, seed=8),
        "dsac_rms": dict(auto=True, n_step=1, bs=64, optim="rms", seed=8),
        "dsac_softmax": dict(auto=False, n_step=1, bs=64, optim="adam", softmax=True,
                             seed=41),
    }
    assert (cfg["E"], cfg["S"], cfg["D"], cfg["A"], cfg["hidden"]) == (6, 40, 12, 6, [16, 16])
    assert (cfg["alpha"], cfg["alpha_lr"], cfg["tau"], cfg["gamma"], cfg["adam_eps"]) == \
        (0.2, 3e-3, 0.05, 0.97, 1e-5)
    assert cfg["target_entropy"] == 0.98 * float(np.log(6))
    assert z["add_act"].dtype == np.int64 and z["add_act"].max() == 5
    for tag, v in cfg["variants"].items():
        assert z[tag + "_indices"].shape == (common.N_UPDATES, v["bs"])
        assert z[tag + "_ent"].shape == z[tag + "_v"].shape == (common.N_UPDATES, v["bs"])
        # the condition gen_dsac asserted: rtol 1e-4 on the outgoing weights is well posed
        assert float(np.abs(z[tag + "_td"]).min()) >= cfg["min_td"] == 1e-2
        for u in range(common.N_UPDATES):  # the recorded magnitudes are those of the parts
            a = float(z[tag + "_alpha_in"][u])
            np.testing.assert_allclose(z[tag + "_mag_alpha_h"][u],
                                       np.abs(a * z[tag + "_ent"][u].astype(np.float64)).mean(),
                                       rtol=1e-6)
            np.testing.assert_allclose(z[tag + "_mag_v"][u],
                                       np.abs(z[tag + "_v"][u].astype(np.float64)).mean(),
                                       rtol=1e-6)
            np.testing.assert_allclose(
                float(z[tag + "_loss_actor"][u]),
                -(a * z[tag + "_ent"][u].astype(np.float64) + z[tag + "_v"][u]).mean(),
                rtol=0, atol=common.actor_loss_bound(z, tag, u))
    # the greedy collect's actions cannot flip on an f32 summation-order difference
    assert z["col_gap"].shape == (30, 4) and float(z["col_gap"].min()) >= 1e-4


def _policy_args(z, dev="cpu"):
    cfg = common.learn_cfg(z)
    nets = common.make_nets(z, cfg, cfg["variants"]["dsac"], dev)
    opt = {n: common.make_optim("adam", m.parameters()) for n, m in nets.items()}
    return cfg, nets, (nets["actor"], opt["actor"], nets["critic1"], opt["critic1"],
                       nets["critic2"], opt["critic2"])


def test_constructor_assertions_and_defaults(z):
    from tianshou_amd.policy import DDPGPolicy, DiscreteSACPolicy, SACPolicy
    cfg, nets, args = _policy_args(z)
    for bad in (-0.1, 1.5):
        with pytest.raises(AssertionError, match="tau should be in"):
            DiscreteSACPolicy(*args, tau=bad)
        with pytest.raises(AssertionError, match="gamma should be in"):
            DiscreteSACPolicy(*args, gamma=bad)
    for log_alpha in (torch.zeros(2, requires_grad=True), torch.zeros(1)):
        with pytest.raises(AssertionError):
            DiscreteSACPolicy(*args, alpha=(1.0, log_alpha, None))
    with pytest.raises(TypeError):  # fixed by the constructor, as in the reference
        DiscreteSACPolicy(*args, action_scaling=True)
    p = DiscreteSACPolicy(*args)
    assert isinstance(p, SACPolicy) and isinstance(p, DDPGPolicy)
    assert (p.tau, p._gamma, p._alpha, p._is_auto_alpha, p._n_step, p._rew_norm, p._noise,
            p._deterministic_eval) == (0.005, 0.99, 0.2, False, 1, False, None, True)
    assert p.action_scaling is False and p.action_bound_method == ""
    assert p.fused and p.fused_adam and p.graph_learn is None and p.eager_collect_step
    assert not hasattr(p, "actor_old") and not hasattr(p, "critic")
    assert p._sync_order == ("critic1", "critic2")
    assert p._optim_order == ("critic1", "critic2", "actor")
    assert not DiscreteSACPolicy(*args, deterministic_eval=False)._deterministic_eval
    log_alpha = torch.full((1,), 0.5, requires_grad=True)
    optim = torch.optim.Adam([log_alpha], lr=3e-3)
    p = DiscreteSACPolicy(*args, alpha=(1.7, log_alpha, optim), estimation_step=3)
    assert p._is_auto_alpha and p._target_entropy == 1.7 and p._log_alpha is log_alpha
    assert p._alpha_optim is optim and p._n_step == 3
    assert torch.equal(p._alpha, log_alpha.detach().exp())
    # an action passes map_action unchanged
    act = np.array([3, 0, 5])
    assert p.map_action(act) is act or np.array_equal(p.map_action(act), act)


def test_train_and_sync_weight_semantics(z):
    from copy import deepcopy
    from tianshou_amd.policy import DiscreteSACPolicy
    cfg, nets, args = _policy_args(z)
    p = DiscreteSACPolicy(*args, tau=0.25)
    assert not p.critic1_old.training and not p.critic2_old.training
    assert p.train(False) is p and not p.training
    assert not (p.actor.training or p.critic1.training or p.critic2.training)
    assert p.train() is p and p.training
    assert p.actor.training and p.critic1.training and p.critic2.training
    assert not p.critic1_old.training and not p.critic2_old.training
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


def test_exploration_noise_is_the_identity(z):
    from tianshou_amd.data import Batch
    from tianshou_amd.policy import DiscreteSACPolicy
    cfg, nets, args = _policy_args(z)
    p = DiscreteSACPolicy(*args)
    for act in (np.array([1, 4, 2]), torch.tensor([0, 5])):
        assert p.exploration_noise(act, Batch()) is act


def test_forward_modes(z):
    from tianshou_amd.data import Batch
    cfg = common.learn_cfg(z)
    obs = torch.as_tensor(z["add_obs"][:200])
    for tag in ("dsac", "dsac_softmax"):
        policy, _ = common.make_policy(z, cfg, tag, "cpu")
        policy.train(False)
        with torch.no_grad():
            res = policy(Batch(obs=obs, info=Batch()))
        assert set(res.keys()) == {"logits", "act", "state", "dist"}
        assert res.state is None and isinstance(res.dist, Categorical)
        assert res.logits.shape == (200, 6)
        assert res.act.dtype == torch.int64 and torch.equal(res.act, res.logits.argmax(-1))
        if tag == "dsac_softmax":  # probabilities, handed to Categorical as logits
            torch.testing.assert_close(res.logits.sum(-1), torch.ones(200), rtol=0, atol=1e-5)
        torch.testing.assert_close(res.dist.logits,
                                   res.logits - res.logits.logsumexp(-1, keepdim=True))
        policy.train()
        torch.manual_seed(5)
        with torch.no_grad():
            res = policy(Batch(obs=obs, info=Batch()))
        assert res.act.dtype == torch.int64 and res.act.shape == (200,)
        assert int(res.act.min()) >= 0 and int(res.act.max()) <= 5
        assert len(set(res.act.tolist())) > 1 and not torch.equal(res.act, res.logits.argmax(-1))
        policy.train(False)
        policy._deterministic_eval = False  # eval mode samples too
        with torch.no_grad():
            res = policy(Batch(obs=obs, info=Batch()))
        assert not torch.equal(res.act, res.logits.argmax(-1))


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
    policy, v = common.make_policy(z, cfg, tag, "cpu", fused=False)
    policy.train()
    ring = HostRing(z, dict(cfg, A=1))  # one integer action per row
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
        batch = Batch(obs=torch.as_tensor(ring.obs[idx]),
                      act=ring.act[idx, 0].astype(np.int64), returns=torch.as_tensor(returns),
                      info=Batch())
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


# -- the kernels' formulas against torch autograd in f64 ------------------------------------------------
def _rows(b, A, seed, softmax=False):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(b, A, generator=g, dtype=torch.float64) * 2.0
    if softmax:
        logits = logits.softmax(-1)
    q1 = torch.randn(b, A, generator=g, dtype=torch.float64) + 1.0
    q2 = torch.randn(b, A, generator=g, dtype=torch.float64) + 1.0
    if b > 2 and A > 1:
        q2[::3] = q1[::3]  # ties
    return logits, q1, q2


@pytest.mark.parametrize("softmax", (False, True))
@pytest.mark.parametrize("b,A", ((1, 1), (3, 2), (65, 6), (33, 18), (7, 65)))
def test_numpy_restatement_matches_torch_autograd_f64(b, A, softmax):
    logits, q1, q2 = _rows(b, A, 100 * b + A, softmax)
    alpha, log_alpha, te = 0.37, -0.8, 0.98 * float(np.log(max(A, 2)))
    # _target_q (discrete_sac.py:93-97)
    dist = Categorical(logits=logits)
    want = (dist.probs * torch.min(q1, q2)).sum(-1) + alpha * dist.entropy()
    np.testing.assert_allclose(common.target64(logits.numpy(), q1.numpy(), q2.numpy(), alpha),
                               want.numpy(), rtol=1e-12, atol=1e-13)
    # the actor and temperature losses (:127-140) with autograd's gradient towards the logits
    x = logits.clone().requires_grad_(True)
    dist = Categorical(logits=x)
    entropy = dist.entropy()
    actor = -(alpha * entropy + (dist.probs * torch.min(q1, q2)).sum(-1)).mean()
    actor.backward()
    la = torch.tensor([log_alpha], dtype=torch.float64, requires_grad=True)
    alpha_loss = -(la * (-entropy.detach() + te)).mean()
    alpha_loss.backward()
    loss, g, a_loss, g_la = common.actor_loss64(logits.numpy(), q1.numpy(), q2.numpy(), alpha,
                                                log_alpha, te)
    np.testing.assert_allclose(loss, actor.item(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(g, x.grad.numpy(), rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(a_loss, alpha_loss.item(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(g_la, la.grad.item(), rtol=1e-12, atol=1e-14)
    if A == 1:
        assert float(np.abs(g).max()) == 0.0
    # the critics' losses (:108-124)
    gen = torch.Generator().manual_seed(b + A)
    act = torch.randint(0, A, (b,), generator=gen)
    returns = torch.randn(b, generator=gen, dtype=torch.float64)
    for weight in (None, torch.rand(b, generator=gen, dtype=torch.float64)):
        xs = [q.clone().requires_grad_(True) for q in (q1, q2)]
        tds, ls = [], []
        for q in xs:
            td = q.gather(1, act[:, None]).flatten() - returns
            ls.append((td.pow(2) * (1.0 if weight is None else weight)).mean())
            ls[-1].backward()
            tds.append(td.detach())
        losses, grads, td = common.q_loss64(q1.numpy(), q2.numpy(), act.numpy(),
                                            returns.numpy(),
                                            None if weight is None else weight.numpy())
        np.testing.assert_allclose(losses, [l.item() for l in ls], rtol=1e-12)
        for gk, q in zip(grads, xs):
            np.testing.assert_allclose(gk, q.grad.numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(td, ((tds[0] + tds[1]) / 2.0).numpy(), rtol=1e-12, atol=0)
