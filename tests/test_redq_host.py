"""tests/golden/redq.npz (tools/gen_goldens.py gen_redq) pinned on the host, and the host parts
of REDQPolicy and EnsembleLinear: the C ABI symbols, the layer's parameters, initialiser and
forward, the constructor's assertions, and the torch leg (``forward``, ``_target_q`` and
``learn`` on the CPU) replaying every recorded variant over tests/test_ddpg_host.py's HostRing.

The replay keeps NumPy's global stream where the reference had it: the buffer's index draws are
restated here (manager.py:163-192; a prioritized buffer draws ``np.random.rand(batch)``), so the
subset draws of ``_target_q`` must come out as recorded.  Tolerances are tests/test_sac_host.py's
for the same quantities: returns rtol 1e-5 / atol 1e-6, critic loss rtol 2e-5, outgoing weights
rtol 1e-4, parameters, log_alpha and alpha rtol 1e-5 / atol 1e-6, actor and temperature losses
by redq_common.actor_loss_bound / alpha_loss_bound."""
import os
import re

import numpy as np
import pytest
import torch

from tests import redq_common as common
from tests.test_ddpg_host import HostRing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("tsrl_redq_target", "tsrl_redq_q_loss_fwd_bwd", "tsrl_redq_actor_loss_fwd_bwd")


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
    assert list(cfg["variants"]) == common.TAGS
    v = cfg["variants"]
    assert cfg["ensemble"] == 5 and cfg["hidden"] == [16, 16]
    assert (v["redq"]["auto"], v["redq"]["subset"], v["redq"]["mode"], v["redq"]["delay"]) == \
        (False, 2, "min", 2)
    assert v["redq_auto"]["auto"] and v["redq_auto"]["delay"] == 3
    assert (v["redq_mean"]["mode"], v["redq_mean"]["subset"]) == ("mean", 3)
    assert (v["redq_full"]["subset"], v["redq_full"]["delay"]) == (5, 1)
    assert v["redq_per"]["per"] and v["redq_per"]["n_step"] == 3
    assert v["redq_rms"]["optim"] == "rms"
    for tag, t in v.items():
        did = z[tag + "_did_actor"]
        assert did.tolist() == [(u + 1) % t["delay"] == 0 for u in range(common.N_UPDATES)]
        assert z[tag + "_subset"].shape == (common.N_UPDATES, t["subset"])
        for u in range(common.N_UPDATES):
            s = z[tag + "_subset"][u]
            assert len(set(s.tolist())) == len(s) and s.min() >= 0 and s.max() < 5
            assert np.isnan(z[tag + "_loss_actor"][u]) == (not did[u])
            assert np.isnan(z[tag + "_eps_learn"][u]).all() == (not did[u])
        assert z[tag + "_q_obs"].shape == (common.N_UPDATES, 5, t["bs"])
        assert np.abs(z[tag + "_eps_target"]).max() <= 2.0
        assert np.abs(z[tag + "_td"]).min() >= cfg["min_td"] == 1e-2  # gen_redq's condition
    assert did.any() and not z["redq_auto_did_actor"].all()  # both step kinds, more than once
    a = z["fwd_train_act"].astype(np.float64)
    assert (1.0 - a * a).min() >= 0.02


# -- EnsembleLinear -----------------------------------------------------------------------------------
def test_ensemble_linear_parameters_and_export():
    from tianshou_amd.utils import net
    from tianshou_amd.utils.net import EnsembleLinear, Linear
    assert net.EnsembleLinear is EnsembleLinear and issubclass(Linear, torch.nn.Linear)
    lin = EnsembleLinear(4, 7, 3)
    sd = lin.state_dict()
    assert list(sd) == ["weight", "bias"]
    assert sd["weight"].shape == (4, 7, 3) and sd["bias"].shape == (4, 1, 3)
    assert lin.weight.requires_grad and lin.bias.requires_grad
    k = float(np.sqrt(1.0 / 7))
    assert float(lin.weight.detach().abs().max()) <= k
    assert float(lin.bias.detach().abs().max()) <= k
    nb = EnsembleLinear(4, 7, 3, bias=False)
    assert nb.bias is None and list(nb.state_dict()) == ["weight"]
    assert nb(torch.ones(2, 7)).shape == (4, 2, 3)


def test_seeded_construction_equals_the_reference(z):
    """The same torch.rand calls in the same order: the ensemble built alone under the recorded
    seed has the reference's weights bit for bit."""
    cfg = common.learn_cfg(z)
    torch.manual_seed(cfg["init_seed"])
    critics = common.make_critics(cfg, "cpu")
    names = [k for k, _ in critics.named_parameters()]
    assert names == [k[len("seeded_critics."):] for k in z if k.startswith("seeded_critics.")]
    for k, p in critics.named_parameters():
        assert np.array_equal(p.detach().numpy(), z["seeded_critics." + k]), k
    # and a state_dict of the reference's loads by name
    sd = {k: torch.as_tensor(z["init_critics." + k]) for k in names}
    missing = critics.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys
    assert all(k.startswith("preprocess.") for k in missing.missing_keys)  # the second name


@pytest.mark.parametrize("bias", (True, False))
def test_ensemble_linear_forward_matches_f64(bias):
    from tianshou_amd.utils.net import EnsembleLinear
    torch.manual_seed(3)
    lin = EnsembleLinear(5, 9, 4, bias=bias)
    w = lin.weight.detach().double()
    c = lin.bias.detach().double() if bias else 0.0
    x2, x3 = torch.randn(11, 9), torch.randn(5, 11, 9)
    y2, y3 = lin(x2), lin(x3)
    assert y2.shape == (5, 11, 4) and y3.shape == (5, 11, 4)
    want2 = torch.einsum("bi,eio->ebo", x2.double(), w) + c
    want3 = torch.einsum("ebi,eio->ebo", x3.double(), w) + c
    torch.testing.assert_close(y2.double(), want2, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(y3.double(), want3, rtol=1e-5, atol=1e-6)
    (y2.sum() + y3.sum()).backward()
    assert lin.weight.grad.shape == (5, 9, 4)
    torch.testing.assert_close(lin.weight.grad.double(), (x2.double().sum(0)[None, :, None]
                               + x3.double().sum(1)[:, :, None]).expand(5, 9, 4),
                               rtol=1e-5, atol=1e-6)
    if bias:
        assert torch.equal(lin.bias.grad, torch.full((5, 1, 4), 22.0))


def test_critic_of_ensemble_layers_gives_E_b_1(z):
    cfg = common.learn_cfg(z)
    critics = common.make_nets(z, cfg, "cpu")["critics"]
    obs, act = z["fwd_obs"], z["fwd_act_in"]
    with torch.no_grad():
        q = critics(obs, act)
    assert q.shape == (cfg["ensemble"], len(obs), 1) == z["fwd_q"].shape
    np.testing.assert_allclose(q.numpy(), z["fwd_q"], rtol=1e-5, atol=1e-6)
    rows = q.flatten(1)
    assert float((rows[0] - rows[1]).abs().max()) > 0  # the members differ


# -- constructor ----------------------------------------------------------------------------------------
def _policy_args(z, dev="cpu"):
    cfg = common.learn_cfg(z)
    nets = common.make_nets(z, cfg, dev)
    opt = {n: common.make_optim("adam", m.parameters()) for n, m in nets.items()}
    return cfg, nets, (nets["actor"], opt["actor"], nets["critics"], opt["critics"])


def test_constructor_assertions_and_defaults(z):
    from tianshou_amd.policy import DDPGPolicy, REDQPolicy, SACPolicy
    cfg, nets, args = _policy_args(z)
    for bad in (-0.1, 1.5):
        with pytest.raises(AssertionError, match="tau should be in"):
            REDQPolicy(*args, tau=bad, action_scaling=False)
        with pytest.raises(AssertionError, match="gamma should be in"):
            REDQPolicy(*args, gamma=bad, action_scaling=False)
    with pytest.raises(AssertionError, match="tanh mapping is not supported"):
        REDQPolicy(*args, action_scaling=False, action_bound_method="tanh")
    for ens, sub in ((5, 0), (5, 6), (2, 3)):
        with pytest.raises(AssertionError, match="Invalid choice of ensemble size or subset"):
            REDQPolicy(*args, ensemble_size=ens, subset_size=sub, action_scaling=False)
    with pytest.raises(ValueError, match="Unsupported mode of Q target computing"):
        REDQPolicy(*args, target_mode="max", action_scaling=False)
    for log_alpha in (torch.zeros(2, requires_grad=True), torch.zeros(1),
                      torch.zeros((), requires_grad=True)):
        with pytest.raises(AssertionError):
            REDQPolicy(*args, alpha=(-3.0, log_alpha, None), action_scaling=False)
    p = REDQPolicy(*args, action_scaling=False)
    assert isinstance(p, DDPGPolicy) and not isinstance(p, SACPolicy)
    assert (p.ensemble_size, p.subset_size, p.tau, p._gamma, p._alpha, p._is_auto_alpha,
            p._n_step, p._rew_norm, p.actor_delay, p._noise, p._deterministic_eval,
            p.target_mode, p.critic_gradient_step) == \
        (10, 2, 0.005, 0.99, 0.2, False, 1, False, 20, None, True, "min", 0)
    assert p.fused and p.fused_adam and p.graph_learn is None and p.eager_collect_step
    assert not hasattr(p, "actor_old") and not hasattr(p, "critic")
    assert p._critic_names == ("critics",) and p._sync_order == ("critics",)
    assert p._optim_order == ("critics", "actor")
    assert not p.critics_old.training
    assert p.train(False) is p and not (p.actor.training or p.critics.training)
    assert p.train() is p and p.actor.training and p.critics.training
    assert not p.critics_old.training
    log_alpha = torch.full((1,), 0.5, requires_grad=True)
    optim = torch.optim.Adam([log_alpha], lr=3e-3)
    p = REDQPolicy(*args, alpha=(-3.0, log_alpha, optim), target_mode="mean",
                   action_scaling=False)
    assert p._is_auto_alpha and p._target_entropy == -3.0 and p._log_alpha is log_alpha
    assert p._alpha_optim is optim and p.target_mode == "mean"
    assert torch.equal(p._alpha, log_alpha.detach().exp())


def test_forward_reproduces_recorded_forwards(z):
    from tianshou_amd.data import Batch
    cfg = common.learn_cfg(z)
    policy, _ = common.make_policy(z, cfg, "redq", "cpu")
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
    policy.train(False)
    with torch.no_grad():
        res = policy(Batch(obs=obs, info=Batch()))  # deterministic_eval: no draw left to take
    assert torch.equal(res.act, torch.tanh(res.logits[0]))


# -- the torch leg against the recording ------------------------------------------------------------
class _ObsNext:
    """What DDPGPolicy._obs_next reads of a buffer."""

    def __init__(self, ring):
        self.ring = ring

    def get(self, indices, key):
        assert key == "obs_next"
        return torch.as_tensor(self.ring.obs_next[indices])


def _sample_indices(z, cfg, v):
    """The np.random calls of the reference's sample_indices, in order.  A VectorReplayBuffer's
    indices come out (manager.py:163-192); a prioritized one draws np.random.rand(batch) and
    descends its tree, so only the stream is advanced (None)."""
    if v.get("per"):
        np.random.rand(v["bs"])
        return None
    lengths = z["buf_lengths"]
    buffer_idx = np.random.choice(cfg["E"], v["bs"], p=lengths / lengths.sum())
    sample_num = np.bincount(buffer_idx, minlength=cfg["E"])
    return np.concatenate([np.random.choice(lengths[b], n) + b * cfg["S"]
                           for b, n in enumerate(sample_num) if n > 0])


@pytest.mark.parametrize("tag", common.TAGS)
def test_torch_leg_replays_recording_on_cpu(z, tag, monkeypatch):
    from tianshou_amd.data import Batch
    cfg = common.learn_cfg(z)
    policy, v = common.make_policy(z, cfg, tag, "cpu")
    policy.train()
    common.feed_draws(policy, common.update_draws(z, tag))
    ring = HostRing(z, cfg)
    stub = _ObsNext(ring)
    subsets, choice = [], np.random.choice

    def spy(*a, **kw):
        res = choice(*a, **kw)
        if kw.get("replace") is False:
            assert a == (cfg["ensemble"], v["subset"])
            subsets.append(res)
        return res

    monkeypatch.setattr(np.random, "choice", spy)
    np.random.seed(v["seed"])
    n_actor = 0
    for u in range(common.N_UPDATES):
        q = f"{tag} update {u}"
        idx = _sample_indices(z, cfg, v)
        if idx is None:
            idx = z[tag + "_indices"][u]
        assert idx.tolist() == z[tag + "_indices"][u].tolist(), q

        def target_q(rows):
            with torch.no_grad():
                return policy._target_q(stub, rows).flatten().numpy()

        returns = ring.nstep(idx, target_q, cfg["gamma"], v["n_step"])
        assert len(subsets) == u + 1 and subsets[u].tolist() == z[tag + "_subset"][u].tolist(), q
        np.testing.assert_allclose(returns, z[tag + "_returns"][u].reshape(-1), rtol=1e-5,
                                   atol=1e-6, err_msg=q)
        batch = Batch(obs=torch.as_tensor(ring.obs[idx]), act=torch.as_tensor(ring.act[idx]),
                      returns=torch.as_tensor(returns), info=Batch())
        if v.get("per"):
            batch.weight = torch.as_tensor(z[tag + "_weight"][u])
        with torch.no_grad():
            q_obs = policy.critics(batch.obs, batch.act).flatten(1).numpy()
        np.testing.assert_allclose(q_obs, z[tag + "_q_obs"][u], rtol=1e-5, atol=1e-6, err_msg=q)
        res = policy.learn(batch)
        did = common.did_actor(z, tag, u)
        n_actor += did
        assert did == ((u + 1) % v["delay"] == 0) and policy.critic_gradient_step == u + 1
        assert set(res) == set(common.loss_keys(v["auto"], did)), q
        np.testing.assert_allclose(res["loss/critics"], float(z[tag + "_loss_critics"][u]),
                                   rtol=2e-5, err_msg=q)
        if did:
            assert isinstance(res["loss/actor"], float)  # the reference: a 1-tuple
            assert abs(res["loss/actor"] - float(z[tag + "_loss_actor"][u])) <= \
                common.actor_loss_bound(z, tag, u), q
        if did and v["auto"]:
            assert abs(res["loss/alpha"] - float(z[tag + "_loss_alpha"][u])) <= \
                common.alpha_loss_bound(z, cfg, tag, u), q
            np.testing.assert_allclose(res["alpha"], float(z[tag + "_alpha"][u]), rtol=1e-5,
                                       atol=1e-6, err_msg=q)
        if v["auto"]:
            np.testing.assert_allclose(policy._log_alpha.detach().numpy(),
                                       z[tag + "_log_alpha"][u], rtol=1e-5, atol=1e-6)
        assert batch.weight.shape == (v["bs"],) and not batch.weight.requires_grad
        np.testing.assert_allclose(batch.weight.numpy(), z[tag + "_td"][u], rtol=1e-4,
                                   err_msg=q)
        np.testing.assert_allclose(common.flat_params(policy), z[tag + "_params"][u],
                                   rtol=1e-5, atol=1e-6, err_msg=q)
    assert n_actor == common.N_UPDATES // v["delay"]
    with pytest.raises(StopIteration):  # one draw per update and one more per actor step
        policy._rsample_noise((1, 1), "cpu")
