"""Fused PPO loss kernel vs the torch fp32 restatement (oracle/ref.py), and PPOPolicy.learn
vs the reference's recorded losses/parameters (tests/golden/ppo_learn.npz).

Tolerances: loss terms rtol 1e-5; gradients rtol 1e-4 / atol 1e-6 (f32 reductions in a
different order than torch's); parameters after Adam steps rtol 1e-3 (GEMMs on the GPU
vs the reference's CPU torch)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import ref

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


# Directed rows: overwritten over the first rows of a random minibatch so that every branch of
# the shared surrogate / value-loss functions (csrc/ppo_loss.h) is taken deterministically.
# B = 257 rows through an index into 294 stored rows: two blocks, a ragged last one.
DIRECTED = dict(eps_clip=0.25, dual_clip=3.0, value_clip=True, norm_adv=False)
DIRECTED_B, DIRECTED_N = 257, 294
# (v, v_s, ret) with eps_clip = 0.25: v - v_s exactly +eps_clip and -eps_clip (clamp passes the
# gradient on the closed interval), an exact tie vf1 == vf2, the unclipped branch wins, the
# clipped branch wins out of range (gradient exactly 0).
VALUE_ROWS = [(0.75, 0.5, 1.0), (0.25, 0.5, 1.0), (0.5, 0.5, 1.0), (1.0, 0.5, 0.0),
              (1.0, 0.5, 1.2)]
# d(vf)/d(v) of VALUE_ROWS (torch's semantics, checked on the CPU): the gradient of the mean
# loss w.r.t. value times B / vf_coef
VALUE_ROWS_DV = [-0.5, -1.5, -1.0, 2.0, 0.0]
# (log ratio, advantage) with lo, hi = 0.75, 1.25 and dual_clip = 3: ratio == 1 exactly (the
# tie surr1 == surr2) for both signs of the advantage, the ratio above hi, above dual_clip
# (ratio > 3 with an < 0 takes clip1 < dual * an) and below lo, each for both signs.
_L2, _L4 = float(np.log(2.0)), float(np.log(4.0))
SURR_ROWS = [(0.0, 1.5), (0.0, -0.75), (_L2, 1.0), (_L2, -1.0), (_L4, 1.0), (_L4, -1.0),
             (-_L2, 1.0), (-_L2, -1.0)]
# SURR_ROWS whose objective has no gradient w.r.t. the ratio (clipped away / dual-clipped)
SURR_ROWS_ZERO_GRAD = [2, 4, 5, 7]


def set_value_rows(value, v_s, ret, idx, first=0):
    for k, (v, vs, rt) in enumerate(VALUE_ROWS):
        value[first + k], v_s[idx[first + k]], ret[idx[first + k]] = v, vs, rt


def set_surrogate_rows(logp_kernel, logp_old, adv, idx, first):
    """logp_kernel [B]: the kernel's own log-prob of the minibatch rows (tsrl_gauss_logp /
    tsrl_cat_logp), so that a log ratio of 0 is exactly 0 in the loss kernel."""
    for k, (log_ratio, a) in enumerate(SURR_ROWS):
        j = idx[first + k]
        logp_old[j] = logp_kernel[first + k] - log_ratio
        adv[j] = a


def check_value_rows(grad_value, B, vf_coef, first=0):
    """One f32 rounding of the f64 product vf_coef * dv / B lies between dv and the stored
    gradient: 2^-24 relative; the out-of-range row's gradient is exactly 0."""
    got = grad_value[first:first + len(VALUE_ROWS)].astype(np.float64) * B / vf_coef
    np.testing.assert_allclose(got, VALUE_ROWS_DV, rtol=1e-6, atol=0)
    assert got[-1] == 0.0


def _kernel_gauss_logp(mu, log_std, act):
    from tianshou_amd import _C
    out = torch.empty(mu.shape[0], dtype=torch.float32, device=mu.device)
    _C.check(_C.lib().tsrl_gauss_logp(_C.ptr(mu), _C.ptr(log_std), _C.ptr(act), mu.shape[0],
                                      mu.shape[1], _C.ptr(out), _C.stream_ptr(mu.device)),
             "tsrl_gauss_logp")
    return out


@pytest.mark.parametrize("kw", CASES)
@pytest.mark.parametrize("B,A", [(4096, 17), (1000, 6), (257, 1)])
def test_fused_loss_vs_torch(dev, kw, B, A):
    _check_fused_loss(dev, kw, B, A)


def test_fused_loss_vs_torch_directed(dev):
    """One more case of test_fused_loss_vs_torch: A = 3 with the directed rows."""
    assert DIRECTED_N == DIRECTED_B + 37
    _check_fused_loss(dev, DIRECTED, DIRECTED_B, 3, directed=True)


def _check_fused_loss(dev, kw, B, A, directed=False):
    from tianshou_amd import _C
    from tianshou_amd.policy.ppo import _GaussPPOLoss
    from tianshou_amd.dist import DataParallel
    g = torch.Generator().manual_seed(B + A)
    n = B + 37
    mu = torch.randn(B, A, generator=g)
    sp = torch.randn(A, 1, generator=g) * 0.3 - 0.5
    value = torch.randn(B, generator=g)
    act = torch.randn(n, A, generator=g)
    logp_old = torch.randn(n, generator=g) * 0.3 - A
    adv = torch.randn(n, generator=g) * 2 + 0.3
    ret = torch.randn(n, generator=g)
    v_s = ret + torch.randn(n, generator=g) * 0.3
    idx = torch.randperm(n, generator=g)[:B]
    # make logp_old close to the current logp so the ratio straddles the clip range
    from torch.distributions import Independent, Normal
    with torch.no_grad():
        lp = Independent(Normal(mu, sp.view(1, -1).exp().expand_as(mu)), 1).log_prob(act[idx])
        logp_old[idx] = lp + torch.randn(B, generator=g) * 0.2
    d = lambda t: t.to(dev).contiguous()
    if directed:
        set_value_rows(value, v_s, ret, idx)
        lpk = _kernel_gauss_logp(d(mu), d(sp.flatten()), d(act[idx])).cpu()
        set_surrogate_rows(lpk, logp_old, adv, idx, first=len(VALUE_ROWS))
    eps_clip = kw.get("eps_clip", 0.2)
    want = ref.ppo_gaussian_loss_torch(
        mu, sp.flatten(), value, act[idx], logp_old[idx], adv[idx], ret[idx], v_s[idx],
        eps_clip=eps_clip, dual_clip=kw.get("dual_clip"), value_clip=kw.get("value_clip", False),
        norm_adv=kw.get("norm_adv", True), vf_coef=0.25, ent_coef=kw.get("ent_coef", 0.01))
    p = _C.PPOParams()
    p.eps_clip, p.dual_clip = eps_clip, kw.get("dual_clip") or 0.0
    p.vf_coef, p.ent_coef, p.adv_eps, p.b_global = 0.25, kw.get("ent_coef", 0.01), 1e-8, B
    p.value_clip, p.norm_adv = int(kw.get("value_clip", False)), int(kw.get("norm_adv", True))
    mu_d = d(mu).requires_grad_(True)
    sp_d = d(sp).requires_grad_(True)
    v_d = d(value).requires_grad_(True)
    loss, terms = _GaussPPOLoss.apply(mu_d, sp_d, v_d, (d(act), d(logp_old), d(adv), d(ret),
                                                         d(v_s), d(idx), p, DataParallel()))
    loss.backward()
    t = terms.cpu().numpy()
    np.testing.assert_allclose(t[1], float(want[1]), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(t[2], float(want[2]), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(t[3], float(want[3]), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(float(loss), float(want[0]), rtol=1e-5, atol=1e-6)
    gw = want[4]
    np.testing.assert_allclose(mu_d.grad.cpu().numpy(), gw["mu"].numpy(), rtol=1e-4,
                               atol=1e-6 * float(gw["mu"].abs().max()) + 1e-9)
    np.testing.assert_allclose(v_d.grad.cpu().numpy(), gw["value"].numpy(), rtol=1e-4,
                               atol=1e-6 * float(gw["value"].abs().max()) + 1e-9)
    np.testing.assert_allclose(sp_d.grad.cpu().numpy().flatten(), gw["sigma_param"].numpy(),
                               rtol=1e-4, atol=1e-6 * float(gw["sigma_param"].abs().max()) + 1e-9)
    if directed:
        check_value_rows(v_d.grad.cpu().numpy(), B, 0.25)
        zero = [len(VALUE_ROWS) + k for k in SURR_ROWS_ZERO_GRAD]
        assert not mu_d.grad[zero].any() and not gw["mu"][zero].any()


@pytest.mark.parametrize("tag", ["base", "multi", "clips", "nonorm"])
def test_learn_matches_reference(golden_dir, dev, tag):
    """PPOPolicy.learn on the reference's fixed weights and batch with the same
    np.random.seed (identical minibatch order): losses and post-Adam parameters."""
    from tianshou_amd.data import Batch
    from tianshou_amd.env import Box
    from tianshou_amd.policy import PPOPolicy
    from tianshou_amd.utils.models import fixed_std_normal, get_actor_critic, init_and_get_optim
    z = np.load(os.path.join(golden_dir, "ppo_learn.npz"))
    p = tag + "_"
    cfg = json.loads(str(z[p + "cfg"]))
    actor, critic = get_actor_critic((17,), (64, 64), (6,), dev)
    optim = init_and_get_optim(actor, critic, 3e-4)
    kw = dict(discount_factor=0.99, gae_lambda=0.95, max_grad_norm=0.5, vf_coef=0.25,
              ent_coef=0.0, reward_normalization=False, advantage_normalization=True,
              eps_clip=0.2, value_clip=False, dual_clip=None)
    kw.update({k: v for k, v in cfg.items() if k not in ("n", "batch_size", "repeat")})
    policy = PPOPolicy(actor, critic, optim, fixed_std_normal,
                       action_space=Box(-1.0, 1.0, (6,)), **kw).to(dev)
    assert policy._fused
    policy.load_state_dict({k[len(p + "init_"):]: torch.as_tensor(z[k]) for k in z.files
                            if k.startswith(p + "init_")})
    t = lambda k: torch.as_tensor(z[p + k], device=dev)
    batch = Batch(obs=t("obs"), act=t("act"), logp_old=t("logp_old"), adv=t("adv"),
                  returns=t("returns"), v_s=t("v_s"))
    np.random.seed(21)
    res = policy.learn(batch, batch_size=cfg["batch_size"], repeat=cfg["repeat"])
    def report(tag, g, w):
        g, w = np.asarray(g, np.float64), np.asarray(w, np.float64)
        e = np.abs(g - w)
        print(f"{p}{tag}: max abs err {e.max():.3g}, max rel err "
              f"{(e / np.maximum(np.abs(w), 1e-30)).max():.3g}")
    for k in ("loss", "loss/clip", "loss/vf", "loss/ent"):
        report(k, res[k], z[p + k.replace("/", "_")])
        # measured (round 3): <= 1.3e-5 rel on the clip term (|clip| ~ 0.02), <= 1e-6 abs
        np.testing.assert_allclose(res[k], z[p + k.replace("/", "_")], rtol=2e-5, atol=1e-6)
    if cfg["repeat"] == 1 and cfg["n"] == cfg["batch_size"]:
        for name, prm in policy.named_parameters():
            key = p + "grad_" + name
            if key in z.files:
                report("grad " + name, prm.grad.cpu().numpy(), z[key])
                np.testing.assert_allclose(prm.grad.cpu().numpy(), z[key], rtol=1e-4,
                                           atol=1e-6)
    sd = policy.state_dict()
    for k in z.files:
        if k.startswith(p + "final_actor.") or k.startswith(p + "final_critic."):
            report(k, sd[k[len(p + "final_"):]].cpu().numpy(), z[k])
            # measured (round 3): <= 5.7e-7 abs after the Adam steps (parameters ~0.1)
            np.testing.assert_allclose(sd[k[len(p + "final_"):]].cpu().numpy(), z[k],
                                       rtol=1e-5, atol=2e-6)


@pytest.mark.parametrize("A", [33, 64, 65])
def test_wide_gaussian_policy(dev, A):
    """get_actor_critic with more action dimensions than the fused MLP takes (32): 33 and 64
    use the fused loss kernel over the torch layers and match a twin on _learn_generic at
    test_learn_matches_reference's tolerances; 65 is wider than the loss kernels too, and
    process_fn and learn() fall back to the generic loop (bit for bit the twin)."""
    import copy
    from tianshou_amd.data import Batch
    from tianshou_amd.env import Box
    from tianshou_amd.policy import PPOPolicy
    from tianshou_amd.utils.models import fixed_std_normal, get_actor_critic, init_and_get_optim
    from . import loss_edges_common as lc
    torch.manual_seed(50 + A)
    actor, critic = get_actor_critic((17,), (64, 64), (A,), dev)
    pols = []
    for a, c in ((actor, critic), (copy.deepcopy(actor), copy.deepcopy(critic))):
        optim = init_and_get_optim(a, c, 3e-4)
        pols.append(PPOPolicy(a, c, optim, fixed_std_normal, action_space=Box(-1.0, 1.0, (A,)),
                              max_grad_norm=0.5, vf_coef=0.25, ent_coef=0.0).to(dev))
    pols[1].load_state_dict(pols[0].state_dict())
    policy, twin = pols
    assert policy._fused and policy._mlp is None
    n = 256
    g = torch.Generator().manual_seed(60 + A)
    obs = torch.randn(n, 17, generator=g).to(dev)
    with torch.no_grad():
        mu = policy.actor.forward_mu(obs)
        sigma = policy.actor.sigma_param.view(1, -1).exp().expand_as(mu)
        act = mu + sigma * torch.randn(n, A, generator=g).to(dev)
        lp = fixed_std_normal(mu, sigma).log_prob(act)
    ret = torch.randn(n, generator=g)
    batch = Batch(obs=obs, act=act, adv=torch.randn(n, generator=g).to(dev), returns=ret.to(dev),
                  v_s=(ret + 0.3 * torch.randn(n, generator=g)).to(dev))
    got = policy._logp_old(batch)  # tsrl_gauss_logp up to 64 dimensions, torch's above
    np.testing.assert_allclose(got.cpu().numpy(), lp.cpu().numpy(), rtol=1e-5, atol=1e-5)
    batch.logp_old = lp + 0.1 * torch.randn(n, generator=g).to(dev)
    generic = lc.count_calls(policy, "_learn_generic")
    np.random.seed(21)
    res = policy.learn(batch, batch_size=64, repeat=2)
    assert len(generic) == (1 if A > 64 else 0)
    np.random.seed(21)
    res_twin = twin._learn_generic(batch, 64, 2)
    keys = ("loss", "loss/clip", "loss/vf", "loss/ent")
    if A > 64:
        assert res == res_twin  # bit for bit: the same code
        for k, v in lc.state_of(policy).items():
            assert torch.equal(v, lc.state_of(twin)[k]), k
    else:
        lc.compare_runs(res, res_twin, lc.state_of(policy), lc.state_of(twin), keys,
                        (2e-5, 1e-6), (1e-5, 2e-6), f"Gaussian A={A}")
