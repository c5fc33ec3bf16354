"""Categorical PPO (discrete actions): the fused tsrl_ppo_cat kernel vs the torch fp32
restatement (oracle/ref.py ppo_categorical_loss_torch), and PPOPolicy.learn /
Categorical log-probs vs the reference's recorded values (tests/golden/ppo_discrete.npz,
tools/gen_goldens.py gen_ppo_discrete).

Tolerances: loss terms rtol 1e-5; gradients rtol 1e-4 / atol 1e-6 * max|grad| (f32
reductions in another order than torch's); log-probs rtol 1e-5; learn() losses rtol 1e-4
and parameters after Adam rtol 1e-3 (GPU GEMMs vs the reference's CPU torch)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import ref

from .test_gpu_ppo import (DIRECTED, DIRECTED_B, DIRECTED_N, VALUE_ROWS, check_value_rows,
                           set_surrogate_rows, set_value_rows)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


CASES = [
    dict(),
    dict(dual_clip=3.0),
    dict(value_clip=True),
    dict(norm_adv=False, ent_coef=0.0),
    dict(dual_clip=5.0, value_clip=True, ent_coef=0.05, eps_clip=0.1),
]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kw", CASES)
@pytest.mark.parametrize("B,A", [(4096, 6), (1000, 2), (257, 18)])
def test_cat_loss_vs_torch(dev, mode, kw, B, A):
    _check_cat_loss(dev, mode, kw, B, A, B + 41)


# after the saturated rows of mode 1
_FIRST = 3


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("A", [2, 6])
def test_cat_loss_vs_torch_directed(dev, mode, A):
    """One more case of test_cat_loss_vs_torch: the directed rows of test_gpu_ppo.py."""
    _check_cat_loss(dev, mode, DIRECTED, DIRECTED_B, A, DIRECTED_N, directed=True)


def _check_cat_loss(dev, mode, kw, B, A, n, directed=False):
    from tianshou_amd import _C
    from tianshou_amd.dist import DataParallel
    from tianshou_amd.policy.ppo import _CatPPOLoss, cat_logp
    g = torch.Generator().manual_seed(B * 3 + A + mode)
    z = torch.randn(B, A, generator=g) * 1.5
    x = z if mode == 0 else torch.softmax(z, -1)
    if mode == 1:  # a few rows with a saturated probability (clamp path of probs_to_logits)
        x[:3] = torch.nn.functional.one_hot(torch.arange(3) % A, A).float()
    value = torch.randn(B, generator=g)
    act = torch.randint(0, A, (n,), generator=g)
    logp_old = torch.randn(n, generator=g)
    adv = torch.randn(n, generator=g) * 2 + 0.3
    ret = torch.randn(n, generator=g)
    v_s = ret + torch.randn(n, generator=g) * 0.3
    idx = torch.randperm(n, generator=g)[:B]
    dist = torch.distributions.Categorical(logits=x) if mode == 0 else \
        torch.distributions.Categorical(probs=x)
    with torch.no_grad():
        logp_old[idx] = dist.log_prob(act[idx]) + torch.randn(B, generator=g) * 0.2
    d = lambda t: t.to(dev).contiguous()  # noqa: E731
    if directed:
        set_value_rows(value, v_s, ret, idx, first=_FIRST)
        lpk = cat_logp(d(x), d(act[idx]), mode).cpu()
        set_surrogate_rows(lpk, logp_old, adv, idx, first=_FIRST + len(VALUE_ROWS))
    eps_clip = kw.get("eps_clip", 0.2)
    want = ref.ppo_categorical_loss_torch(
        x, value, act[idx], logp_old[idx], adv[idx], ret[idx], v_s[idx], mode,
        eps_clip=eps_clip, dual_clip=kw.get("dual_clip"), value_clip=kw.get("value_clip", False),
        norm_adv=kw.get("norm_adv", True), vf_coef=0.25, ent_coef=kw.get("ent_coef", 0.01))
    p = _C.PPOParams()
    p.eps_clip, p.dual_clip = eps_clip, kw.get("dual_clip") or 0.0
    p.vf_coef, p.ent_coef, p.adv_eps, p.b_global = 0.25, kw.get("ent_coef", 0.01), 1e-8, B
    p.value_clip, p.norm_adv = int(kw.get("value_clip", False)), int(kw.get("norm_adv", True))
    x_d = d(x).requires_grad_(True)
    v_d = d(value).requires_grad_(True)
    loss, terms = _CatPPOLoss.apply(x_d, v_d, (d(act), d(logp_old), d(adv), d(ret), d(v_s),
                                               d(idx), p, DataParallel(), mode))
    loss.backward()
    t = terms.cpu().numpy()
    for i in range(1, 4):
        np.testing.assert_allclose(t[i], float(want[i]), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(float(loss), float(want[0]), rtol=1e-5, atol=1e-6)
    gw = want[4]
    np.testing.assert_allclose(x_d.grad.cpu().numpy(), gw["x"].numpy(), rtol=1e-4,
                               atol=1e-6 * float(gw["x"].abs().max()) + 1e-9)
    np.testing.assert_allclose(v_d.grad.cpu().numpy(), gw["value"].numpy(), rtol=1e-4,
                               atol=1e-6 * float(gw["value"].abs().max()) + 1e-9)
    lp = cat_logp(d(x), d(act[idx]), mode).cpu()
    np.testing.assert_allclose(lp.numpy(), dist.log_prob(act[idx]).numpy(), rtol=1e-5,
                               atol=1e-6)
    if directed:
        check_value_rows(v_d.grad.cpu().numpy(), B, 0.25, first=_FIRST)


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


@pytest.mark.parametrize("value_clip", [False, True])
def test_value_loss_same_bits_gauss_and_cat(dev, value_clip):
    """The Gaussian and the Categorical loss kernel give byte-identical value gradients and
    value-loss terms on the same value / ret / v_s / idx: both reduce 256-row blocks in the
    same fixed order, so only the one value_loss definition of csrc/ppo_loss.h lies between
    these inputs and outputs."""
    from tianshou_amd import _C
    from tianshou_amd.dist import DataParallel
    from tianshou_amd.policy.ppo import _CatPPOLoss, _GaussPPOLoss
    g = torch.Generator().manual_seed(5)
    B, n = DIRECTED_B, DIRECTED_N
    value = torch.randn(B, generator=g)
    ret = torch.randn(n, generator=g)
    v_s = ret + torch.randn(n, generator=g) * 0.3
    adv = torch.randn(n, generator=g) * 2 + 0.3
    logp_old = torch.randn(n, generator=g) * 0.3 - 3
    idx = torch.randperm(n, generator=g)[:B]
    set_value_rows(value, v_s, ret, idx)
    mu, sp = torch.randn(B, 3, generator=g), torch.randn(3, 1, generator=g) * 0.3 - 0.5
    act_g = torch.randn(n, 3, generator=g)
    x = torch.randn(B, 6, generator=g) * 1.5
    act_c = torch.randint(0, 6, (n,), generator=g)
    p = _C.PPOParams()
    p.eps_clip, p.dual_clip = DIRECTED["eps_clip"], DIRECTED["dual_clip"]
    p.vf_coef, p.ent_coef, p.adv_eps, p.b_global = 0.25, 0.01, 1e-8, B
    p.value_clip, p.norm_adv = int(value_clip), 0
    d = lambda t: t.to(dev).contiguous()  # noqa: E731
    shared = (d(logp_old), d(adv), d(ret), d(v_s), d(idx), p, DataParallel())
    vg, vc = d(value).requires_grad_(True), d(value).requires_grad_(True)
    loss_g, terms_g = _GaussPPOLoss.apply(d(mu).requires_grad_(True), d(sp).requires_grad_(True),
                                          vg, (d(act_g),) + shared)
    loss_g.backward()
    loss_c, terms_c = _CatPPOLoss.apply(d(x).requires_grad_(True), vc,
                                        (d(act_c),) + shared + (0,))
    loss_c.backward()
    assert _bits(vg.grad) == _bits(vc.grad)
    assert _bits(terms_g[2]) == _bits(terms_c[2])
    assert np.isfinite(vg.grad.cpu().numpy()).all() and vg.grad.abs().max() > 0
    if value_clip:
        check_value_rows(vg.grad.cpu().numpy(), B, 0.25)



def test_cat_loss_seed_paths(dev):
    """_CatPPOLoss's backward under the learn path's constant unit seed (the kernel's
    gradients handed over as they are, round 6) equals loss.backward()'s (x * 1.0 is x, bit
    for bit), and any other seed still scales them (2.5 * loss)."""
    from tianshou_amd import _C
    from tianshou_amd.dist import DataParallel
    from tianshou_amd.policy.ppo import _CatPPOLoss, _unit_seed
    g = torch.Generator().manual_seed(11)
    B, A, n = 96, 6, 137
    x = torch.randn(B, A, generator=g)
    value = torch.randn(B, generator=g)
    act = torch.randint(0, A, (n,), generator=g)
    logp_old, adv, ret = (torch.randn(n, generator=g) for _ in range(3))
    v_s = ret + 0.3 * torch.randn(n, generator=g)
    idx = torch.randperm(n, generator=g)[:B]
    p = _C.PPOParams()
    p.eps_clip, p.dual_clip, p.vf_coef, p.ent_coef, p.adv_eps, p.b_global = \
        0.2, 0.0, 0.25, 0.01, 1e-8, B
    p.value_clip, p.norm_adv = 1, 1
    d = lambda t: t.to(dev).contiguous()  # noqa: E731
    args = (d(act), d(logp_old), d(adv), d(ret), d(v_s), d(idx), p, DataParallel(), 0)
    grads = []
    for seed in ("ones", "unit", 2.5):
        x_d, v_d = d(x).requires_grad_(True), d(value).requires_grad_(True)
        loss, _ = _CatPPOLoss.apply(x_d, v_d, args)
        if seed == "ones":
            loss.backward()
        elif seed == "unit":
            loss.backward(_unit_seed(loss.device))
        else:
            (loss * seed).backward()
        grads.append((x_d.grad.clone(), v_d.grad.clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    torch.testing.assert_close(grads[2][0], 2.5 * grads[0][0], rtol=1e-6, atol=0)
    torch.testing.assert_close(grads[2][1], 2.5 * grads[0][1], rtol=1e-6, atol=0)

def _discrete_policy(z, tag, dev):
    from tianshou_amd.env import Discrete
    from tianshou_amd.policy import PPOPolicy
    from tianshou_amd.utils.net import ActorCritic, DiscreteActor, DiscreteCritic, Net
    cfg = json.loads(str(z[tag + "_cfg"]))
    net = Net(cfg["obs"], hidden_sizes=(64, 64), device=dev)
    actor = DiscreteActor(net, cfg["act"], softmax_output=cfg["softmax"], device=dev).to(dev)
    critic = DiscreteCritic(Net(cfg["obs"], hidden_sizes=(64, 64), device=dev),
                            device=dev).to(dev)
    optim = torch.optim.Adam(ActorCritic(actor, critic).parameters(), lr=1e-3)
    dist = torch.distributions.Categorical if cfg["softmax"] else \
        (lambda q: torch.distributions.Categorical(logits=q))
    kw = dict(discount_factor=0.99, gae_lambda=0.95, max_grad_norm=0.5, vf_coef=0.5,
              eps_clip=0.2, advantage_normalization=True, action_scaling=False)
    kw.update({k: v for k, v in cfg.items()
               if k not in ("n", "batch_size", "repeat", "obs", "act", "softmax")})
    policy = PPOPolicy(actor, critic, optim, dist, action_space=Discrete(cfg["act"]),
                       **kw).to(dev)
    policy.load_state_dict({k[len(tag + "_init_"):]: torch.as_tensor(z[k]) for k in z.files
                            if k.startswith(tag + "_init_")})
    return policy, cfg


@pytest.mark.parametrize("tag", ["probs", "logits", "logits_multi"])
def test_learn_discrete_matches_reference(golden_dir, dev, tag):
    """PPOPolicy.learn (Categorical, fused loss) on the reference's fixed weights and batch
    with the same np.random.seed (identical minibatch order)."""
    from tianshou_amd.data import Batch
    z = np.load(os.path.join(golden_dir, "ppo_discrete.npz"))
    policy, cfg = _discrete_policy(z, tag, dev)
    assert policy._cat == (1 if cfg["softmax"] else 0)
    p = tag + "_"
    t = lambda k: torch.as_tensor(z[p + k], device=dev)  # noqa: E731
    lp = policy._logp_cat(t("obs"), t("act"))
    np.testing.assert_allclose(lp.cpu().numpy(), z[p + "logp_fresh"], rtol=1e-5, atol=1e-6)
    batch = Batch(obs=t("obs"), act=t("act"), logp_old=t("logp_old"), adv=t("adv"),
                  returns=t("returns"), v_s=t("v_s"))
    np.random.seed(21)
    res = policy.learn(batch, batch_size=cfg["batch_size"], repeat=cfg["repeat"])
    for k in ("loss", "loss/clip", "loss/vf", "loss/ent"):
        np.testing.assert_allclose(res[k], z[p + k.replace("/", "_")], rtol=1e-4, atol=1e-5)
    sd = policy.state_dict()
    for k in z.files:
        if k.startswith(p + "final_actor.") or k.startswith(p + "final_critic."):
            # measured (round 3): <= 2.1e-7 abs after the Adam steps (round 2: 1e-3 / 1e-5)
            np.testing.assert_allclose(sd[k[len(p + "final_"):]].cpu().numpy(), z[k],
                                       rtol=1e-5, atol=1e-6)


# -- masked and wide Categorical policies (tests/loss_edges_common.py) --------------------------
def test_learn_masked_actor_matches_generic(dev):
    """An actor that writes -inf over illegal actions, PPOPolicy.learn on the fused Categorical
    path (eager first epoch, graph replay after it) against a twin with the same weights and
    seed on _learn_generic: every parameter finite, losses and parameters at
    test_learn_discrete_matches_reference's tolerances."""
    from tianshou_amd.policy import PPOPolicy
    from . import loss_edges_common as lc
    policy, twin = lc.discrete_policy(PPOPolicy, dev, lambda: lc.MaskedActor(dev), 6, seed=31)
    assert policy._cat == 0 and not policy._fused
    batch = lc.discrete_batch(policy, dev, 200, 6, seed=32, illegal=lc.MASKED_ACTIONS)
    with torch.no_grad():
        x = policy.actor(batch.obs)[0]
    assert bool(torch.isinf(x).any()) and bool(torch.isfinite(x[torch.arange(200), batch.act]).all())
    fused = lc.count_calls(policy, "_learn_cat")
    np.random.seed(21)
    res = policy.learn(batch, batch_size=64, repeat=2)
    assert fused == ["_learn_cat"]
    np.random.seed(21)
    res_twin = twin._learn_generic(batch, 64, 2)
    print("masked PPO losses:", res["loss"])
    lc.compare_runs(res, res_twin, lc.state_of(policy), lc.state_of(twin),
                    ("loss", "loss/clip", "loss/vf", "loss/ent"), (1e-4, 1e-5), (1e-5, 1e-6),
                    "masked PPO")


@pytest.mark.parametrize("n_act", [64, 65, 100])
def test_wide_categorical_policy(dev, n_act):
    """More actions than the loss kernels take (64): process_fn and learn() run the torch
    formulation, bit for bit the twin's forced onto _learn_generic (the same code); 64 actions
    still take the fused path."""
    from tianshou_amd.policy import PPOPolicy
    from tianshou_amd.utils.net import DiscreteActor, Net
    from . import loss_edges_common as lc
    make = lambda: DiscreteActor(Net(8, hidden_sizes=(64, 64), device=dev), n_act,  # noqa: E731
                                 softmax_output=False, device=dev)
    policy, twin = lc.discrete_policy(PPOPolicy, dev, make, n_act, seed=33)
    assert policy._cat == 0
    runs = []
    for pol in (policy, twin):
        buf = lc.filled_buffer(dev, 8, 25, 8, lambda rng, E: rng.randint(0, n_act, E), seed=34)
        batch, idx = buf.sample(0)
        batch = pol.process_fn(batch, buf, idx)
        with torch.no_grad():
            lp = lc.cat_logits(pol.actor(batch.obs)[0]).log_prob(batch.act)
        np.testing.assert_allclose(batch.logp_old.cpu().numpy(), lp.cpu().numpy(), rtol=1e-5,
                                   atol=1e-6)
        generic, fused = lc.count_calls(pol, "_learn_generic"), lc.count_calls(pol, "_learn_cat")
        np.random.seed(21)
        if pol is policy:
            res = pol.learn(batch, batch_size=64, repeat=2)
            assert (len(generic), len(fused)) == ((0, 1) if n_act <= 64 else (1, 0))
        else:
            res = pol._learn_generic(batch, 64, 2)
        assert all(np.isfinite(res[k]).all() for k in res)
        runs.append((res, lc.state_of(pol)))
    if n_act > 64:
        assert runs[0][0] == runs[1][0]  # bit for bit
        for k, v in runs[0][1].items():
            assert torch.equal(v, runs[1][1][k]), k
    else:
        lc.compare_runs(runs[0][0], runs[1][0], runs[0][1], runs[1][1],
                        ("loss", "loss/clip", "loss/vf", "loss/ent"), (1e-4, 1e-5), (1e-5, 1e-6),
                        "64 actions")
