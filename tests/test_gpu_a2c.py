"""A2CPolicy on the fused device paths: the loss kernels at objective = 1 against torch fp32,
the whole fused minibatch against fp64 autograd, learn() / update() against the reference's
recorded run (tests/golden/a2c.npz, tools/gen_goldens.py gen_a2c), graph replay against eager
launches, and that the fused paths are the ones taken.

Tolerances: loss terms rtol 1e-5, gradients rtol 1e-4 (atol as tests/test_gpu_ppo.py); the
fused minibatch's gradients within max(4 x torch-fp32's error, 2e-6) of fp64 in relative L2;
learn() with Adam at DESIGN.md section 4's losses rtol 2e-5 / atol 1e-6, parameters rtol 1e-5
/ atol 1e-6, gradients rtol 1e-4 / atol 1e-6.  With RMSprop the parameter bound is 4 x what
torch autograd + torch.optim.RMSprop deviate from the same recording on the same GPU
(GENERIC_DEV below)."""
import numpy as np
import pytest
import torch
from torch.distributions import Categorical, Independent, Normal

from tests import a2c_common as common

pytestmark = pytest.mark.gpu

VF, ENT = 0.5, 0.01

# max |parameter - recorded| of the generic A2CPolicy.learn (torch autograd, clip_grad_norm_,
# torch.optim.RMSprop -- the loop the fused paths replace, measured at the commit before them)
# on an MI355X against tests/golden/a2c.npz; sched: after each of the three updates.  An early
# RMSprop step is lr * g / (0.1 |g| + eps): where |g| ~ eps it moves with the last bits of g.
GENERIC_DEV = {
    "rms": 5.96e-8,
    "rms_multi": 1.04e-7,
    "cat_logits": 1.19e-7,
    "sched": (1.30e-7, 1.29e-7, 1.42e-7),
}
# The fused paths measured 1.31e-7, 3.20e-7, 6.7e-8 and (2.02e-7, 2.04e-7, 2.45e-7) in the same
# session; the Adam variants 3.0e-8 (adam_noclip) and 6.0e-8 (cat_probs), generic 3.0e-8 both.


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _params(B, **kw):
    from tianshou_amd import _C
    p = _C.PPOParams()
    p.objective = _C.OBJ_A2C
    p.vf_coef, p.ent_coef, p.adv_eps, p.b_global = VF, ENT, 1e-8, float(B)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _a2c_loss(dist, value, act, adv, ret):
    """a2c.py:126-137."""
    log_prob = dist.log_prob(act).reshape(len(adv), -1).transpose(0, 1)
    actor_loss = -(log_prob * adv).mean()
    vf_loss = torch.nn.functional.mse_loss(ret, value)
    ent = dist.entropy().mean()
    return actor_loss + VF * vf_loss - ENT * ent, actor_loss, vf_loss, ent


def _close(got, want, rtol, what):
    want = want.detach()
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.numpy(), rtol=rtol,
                               atol=1e-6 * float(want.abs().max()) + 1e-9, err_msg=what)


@pytest.mark.parametrize("B,A", [(4096, 17), (1000, 6), (257, 1)])
def test_gauss_loss_a2c_vs_torch(dev, B, A):
    from tianshou_amd.dist import DataParallel
    from tianshou_amd.policy.onpolicy import _GaussPPOLoss
    g = torch.Generator().manual_seed(B + A)
    n = B + 37
    mu = torch.randn(B, A, generator=g).requires_grad_(True)
    sp = (torch.randn(A, 1, generator=g) * 0.3 - 0.5).requires_grad_(True)
    value = torch.randn(B, generator=g).requires_grad_(True)
    act = torch.randn(n, A, generator=g)
    adv = torch.randn(n, generator=g) * 2 + 0.3
    ret = torch.randn(n, generator=g)
    idx = torch.randperm(n, generator=g)[:B]
    dist = Independent(Normal(mu, sp.view(1, -1).exp().expand_as(mu)), 1)
    want = _a2c_loss(dist, value, act[idx], adv[idx], ret[idx])
    want[0].backward()
    d = lambda t: t.detach().to(dev).contiguous()  # noqa: E731
    mu_d, sp_d, v_d = (d(t).requires_grad_(True) for t in (mu, sp, value))
    loss, terms = _GaussPPOLoss.apply(mu_d, sp_d, v_d, (d(act), None, d(adv), d(ret), None,
                                                         d(idx), _params(B), DataParallel()))
    loss.backward()
    t = terms.cpu().numpy()
    for i in range(4):
        np.testing.assert_allclose(t[i], float(want[i]), rtol=1e-5, atol=1e-6)
    _close(mu_d.grad, mu.grad, 1e-4, "mu")
    _close(v_d.grad, value.grad, 1e-4, "value")
    _close(sp_d.grad, sp.grad, 1e-4, "sigma_param")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("B,A", [(4096, 6), (1000, 2), (257, 18)])
def test_cat_loss_a2c_vs_torch(dev, mode, B, A):
    from tianshou_amd.dist import DataParallel
    from tianshou_amd.policy.onpolicy import _CatPPOLoss
    g = torch.Generator().manual_seed(B * 3 + A + mode)
    n = B + 41
    zz = torch.randn(B, A, generator=g) * 1.5
    x = zz if mode == 0 else torch.softmax(zz, -1)
    if mode == 1:  # a few rows with a saturated probability (clamp path of probs_to_logits)
        x[:3] = torch.nn.functional.one_hot(torch.arange(3) % A, A).float()
    x.requires_grad_(True)
    value = torch.randn(B, generator=g).requires_grad_(True)
    act = torch.randint(0, A, (n,), generator=g)
    adv = torch.randn(n, generator=g) * 2 + 0.3
    ret = torch.randn(n, generator=g)
    idx = torch.randperm(n, generator=g)[:B]
    dist = Categorical(logits=x) if mode == 0 else Categorical(probs=x)
    want = _a2c_loss(dist, value, act[idx], adv[idx], ret[idx])
    want[0].backward()
    d = lambda t: t.detach().to(dev).contiguous()  # noqa: E731
    x_d, v_d = d(x).requires_grad_(True), d(value).requires_grad_(True)
    loss, terms = _CatPPOLoss.apply(x_d, v_d, (d(act), None, d(adv), d(ret), None, d(idx),
                                               _params(B), DataParallel(), mode))
    loss.backward()
    t = terms.cpu().numpy()
    for i in range(4):
        np.testing.assert_allclose(t[i], float(want[i]), rtol=1e-5, atol=1e-6)
    _close(x_d.grad, x.grad, 1e-4, "x")
    _close(v_d.grad, value.grad, 1e-4, "value")


@pytest.mark.parametrize("bad", [dict(norm_adv=1), dict(value_clip=1), dict(dual_clip=3.0)])
def test_a2c_objective_rejects_ppo_options(dev, bad):
    """objective = 1 with norm_adv, value_clip or dual_clip is the argument error in all three
    entries; an unknown objective too."""
    from tianshou_amd import _C
    from tianshou_amd.dist import DataParallel
    from tianshou_amd.policy import fused_mlp
    from tianshou_amd.policy.onpolicy import _CatPPOLoss, _GaussPPOLoss
    from tianshou_amd.utils.net import ActorCritic
    B, A = 64, 3
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    sums = torch.zeros(2, dtype=torch.float64, device=dev)
    for p in (_params(B, **bad), _params(B, objective=2)):
        with pytest.raises(_C.TsrlError):
            _GaussPPOLoss.apply(z(B, A), z(A, 1), z(B), (z(B, A), None, z(B), z(B), z(B), None,
                                                         p, DataParallel()))
        with pytest.raises(_C.TsrlError):
            _CatPPOLoss.apply(z(B, A), z(B), (z(B).long(), None, z(B), z(B), z(B), None, p,
                                              DataParallel(), 0))
    from tests.test_gpu_mlp import _nets
    actor, critic = _nets(8, A, dev, 1)
    fm = fused_mlp.FusedActorCritic(fused_mlp.match(actor, critic),
                                    ActorCritic(actor, critic).parameters())
    with pytest.raises(_C.TsrlError):
        fm.minibatch(z(B, 8), None, B, z(B, A), None, z(B), z(B), z(B), _params(B, **bad),
                     DataParallel(), adv_sums=sums)


def _ref_minibatch_a2c(W, obs, act, adv, ret, dtype, device):
    """a2c.py:122-137 on the functional form of get_actor_critic's networks."""
    P = {k: v.detach().to(device, dtype).clone().requires_grad_(True) for k, v in W.items()}
    x = obs.to(device, dtype)
    c = lambda t: t.to(device, dtype)  # noqa: E731
    ha = torch.tanh(torch.tanh(x @ P["w1a"].T + P["b1a"]) @ P["w2a"].T + P["b2a"])
    mu = ha @ P["w3a"].T + P["b3a"]
    hc = torch.tanh(torch.tanh(x @ P["w1c"].T + P["b1c"]) @ P["w2c"].T + P["b2c"])
    value = (hc @ P["w3c"].T + P["b3c"]).flatten()
    sigma = (P["sigma"].view(1, -1) + torch.zeros_like(mu)).exp()
    terms = _a2c_loss(Independent(Normal(mu, sigma), 1), value, c(act), c(adv), c(ret))
    terms[0].backward()
    return (torch.stack(terms).detach().cpu().double(),
            {k: v.grad.detach().cpu().double() for k, v in P.items()})


# fewer rows than one 16-row tile; D % 4 != 0 with a partial tile and a partial 128-row
# workgroup; the maximum action width twice; the headline width
@pytest.mark.parametrize("D,A,B", [(8, 1, 5), (17, 6, 257), (24, 5, 1000), (64, 32, 4096),
                                   (376, 17, 2048)])
def test_fused_minibatch_a2c_matches_autograd(dev, D, A, B):
    from tianshou_amd.dist import DataParallel
    from tianshou_amd.policy import fused_mlp
    from tianshou_amd.utils.net import ActorCritic
    from tests.test_gpu_mlp import _nets
    actor, critic = _nets(D, A, dev, D + A + B)
    layers = fused_mlp.match(actor, critic)
    assert layers is not None
    fm = fused_mlp.FusedActorCritic(layers, ActorCritic(actor, critic).parameters())
    g = torch.Generator().manual_seed(B)
    n = B + 101
    obs = torch.randn(n, D, generator=g).to(dev)
    act = torch.randn(n, A, generator=g).to(dev)
    adv = (torch.randn(n, generator=g) * 2 + 0.3).to(dev)
    ret = torch.randn(n, generator=g).to(dev)
    idx = torch.randperm(n, generator=g)[:B].to(dev)
    W = {"w1a": layers["w1a"].weight, "b1a": layers["w1a"].bias,
         "w2a": layers["w2a"].weight, "b2a": layers["w2a"].bias,
         "w3a": layers["w3a"].weight, "b3a": layers["w3a"].bias,
         "w1c": layers["w1c"].weight, "b1c": layers["w1c"].bias,
         "w2c": layers["w2c"].weight, "b2c": layers["w2c"].bias,
         "w3c": layers["w3c"].weight, "b3c": layers["w3c"].bias,
         "sigma": layers["sigma"]}
    terms = fm.minibatch(fm.rows(obs), idx, B, act, None, adv, ret, None, _params(B),
                         DataParallel())
    torch.cuda.synchronize()
    got = {k: v.grad.detach().cpu().double() for k, v in W.items()}
    mb = [t[idx] for t in (obs, act, adv, ret)]
    t64, g64 = _ref_minibatch_a2c(W, *mb, torch.float64, "cpu")
    t32, g32 = _ref_minibatch_a2c(W, *mb, torch.float32, dev)
    np.testing.assert_allclose(terms.cpu().double().numpy(), t64.numpy(), rtol=1e-5, atol=1e-6)
    for k in W:
        ref = g64[k]
        den = ref.norm().item() + 1e-30
        e_fused = (got[k] - ref).norm().item() / den
        e_torch = (g32[k] - ref).norm().item() / den
        print(f"B={B} {k}: rel L2 err fused {e_fused:.3g}, torch f32 {e_torch:.3g}")
        assert e_fused <= max(4 * e_torch, 2e-6), (k, e_fused, e_torch)


def _assert_fused_storage(policy):
    """Every parameter and every optimiser moment is a view into the flat buffers."""
    flat = policy._mlp if policy._mlp is not None else policy._cat_adam
    assert flat is not None and flat.adam_bound(policy.optim)
    st = flat._adam

    def inside(t, buf):
        return buf.data_ptr() <= t.data_ptr() < buf.data_ptr() + buf.numel() * 4

    name = st["names"][-1]
    for p in policy._actor_critic.parameters():
        assert inside(p, st["p"]) and inside(p.grad, flat.flat_grad)
        assert inside(policy.optim.state[p][name], st["flats"][-1])
    return st["kind"]


def _check_params(policy, want, bound_of):
    sd = policy._actor_critic.state_dict()
    for k, a in want.items():
        got = sd[k].detach().cpu().numpy()
        e = np.abs(got.astype(np.float64) - a)
        print(f"{k}: max abs err {e.max():.3g}")
        bound_of(got, a, k)


def _adam_bound(got, want, k):
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6, err_msg=k)


def _rms_bound(dev_generic):
    def check(got, want, k):
        assert np.abs(got.astype(np.float64) - want).max() <= 4 * dev_generic, k
    return check


@pytest.mark.parametrize("tag", common.LEARN_TAGS)
def test_learn_matches_reference(golden_dir, dev, tag):
    """A2CPolicy.learn on the reference's nets and batch under the same np.random.seed: the
    four reference keys, losses, single-minibatch gradients and final parameters; the fused
    storage is bound and the RandomState ends where the reference's leaves it.

    Measured on an MI355X, max |parameter - recorded| with RMSprop: generic loop 5.96e-8 (rms),
    1.04e-7 (rms_multi), 1.19e-7 (cat_logits); fused paths 1.31e-7, 3.20e-7, 6.7e-8, inside
    the 4 x bound (GENERIC_DEV).  This test prints its own figures."""
    z = common.golden(golden_dir)
    policy, cfg = common.build_policy(z, tag, dev)
    assert (policy._mlp is not None) == (cfg["net"] == "gauss")
    assert (policy._cat is not None) == (cfg["net"] == "cat")
    np.random.seed(21)
    res = policy.learn(common.learn_batch(z, tag, dev), batch_size=cfg["batch_size"],
                       repeat=cfg["repeat"])
    end = np.random.get_state()
    assert tuple(res) == common.KEYS
    kind = _assert_fused_storage(policy)
    assert kind == ("rmsprop" if cfg["optim"] == "rms" else "adam")
    for k in common.KEYS:
        want = z[tag + "_" + k.replace("/", "_")]
        assert len(res[k]) == len(want) and all(isinstance(v, float) for v in res[k])
        e = np.abs(np.asarray(res[k]) - want)
        print(f"{tag} {k}: max abs err {e.max():.3g}")
        np.testing.assert_allclose(res[k], want, rtol=2e-5, atol=1e-6, err_msg=k)
    if cfg["batch_size"] >= cfg["n"]:
        for name, g in common.recorded(z, tag + "_grad_").items():
            np.testing.assert_allclose(common.grad_of(policy._actor_critic, name).cpu().numpy(),
                                       g, rtol=1e-4, atol=1e-6, err_msg=name)
    bound = _rms_bound(GENERIC_DEV[tag]) if cfg["optim"] == "rms" else _adam_bound
    _check_params(policy, common.recorded(z, tag + "_final__actor_critic."), bound)
    np.random.seed(21)
    for _ in range(cfg["repeat"]):
        np.random.permutation(cfg["n"])
    now = np.random.get_state()
    assert end[2] == now[2] and (end[1] == now[1]).all()


def test_sched_updates_match_reference(golden_dir, dev):
    """Three policy.update() calls on the recorded buffer under the LambdaLR of
    examples/mujoco/mujoco_a2c.py:118-127: process_fn's v_s / returns / adv at
    test_process_fn_matches_reference's tolerances (and no log-prob computed), parameters after
    each update within 4 x the generic loop's deviation, the epoch replayed from one captured
    graph from the second update on although the learning rate changes."""
    z = common.golden(golden_dir)
    policy, cfg = common.build_policy(z, "sched", dev)
    M = cfg["max_update_num"]
    policy.lr_scheduler = torch.optim.lr_scheduler.LambdaLR(policy.optim,
                                                            lr_lambda=lambda e: 1 - e / M)
    buf = common.sched_buffer(z, dev)
    seen = []
    process_fn = policy.process_fn

    def recording(batch, buffer, indices):
        batch = process_fn(batch, buffer, indices)
        seen.append({k: batch[k].detach().cpu().numpy() for k in ("v_s", "returns", "adv")})
        assert policy._pending_logp is None and "logp_old" not in batch
        return batch

    policy.process_fn = recording
    np.random.seed(8)
    graphs = []
    for u in range(3):
        res = policy.update(0, buf, batch_size=cfg["bs"], repeat=1)
        for k, got in seen[u].items():
            want = z[f"sched_u{u}_{k}"]
            np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6 * np.abs(want).max(),
                                       err_msg=f"update {u} {k}")
        for k in common.KEYS:
            np.testing.assert_allclose(res[k], z[f"sched_u{u}_" + k.replace("/", "_")],
                                       rtol=2e-5, atol=1e-6, err_msg=f"update {u} {k}")
        assert policy.optim.param_groups[0]["lr"] == float(z[f"sched_u{u}_lr"])
        _check_params(policy, common.recorded(z, f"sched_u{u}_param__actor_critic."),
                      _rms_bound(GENERIC_DEV["sched"][u]))
        graphs.append(policy._learn_graph["graph"] if policy._learn_graph else None)
    assert graphs[1] is not None and graphs[1] is graphs[2]
    assert graphs[0] is None or graphs[0] is graphs[1]
    assert _assert_fused_storage(policy) == "rmsprop"


@pytest.mark.parametrize("tag", ["rms_multi", "cat_probs", "cat_logits"])
def test_learn_graph_replay_matches_eager(golden_dir, dev, tag):
    """The same policy with graph_learn True and False (Gaussian fused MLP; Categorical with
    Adam and with RMSprop): bitwise-equal losses and parameters after two learn() calls."""
    z = common.golden(golden_dir)
    runs = []
    for graph in (True, False):
        policy, cfg = common.build_policy(z, tag, dev)
        policy.graph_learn = graph
        batch = common.learn_batch(z, tag, dev)
        np.random.seed(3)
        out = [policy.learn(batch, batch_size=cfg["batch_size"], repeat=2) for _ in range(2)]
        assert (policy._learn_graph is not None) == graph
        runs.append((out, {k: v.detach().cpu() for k, v in policy.state_dict().items()}))
    for a, b in zip(runs[0][0], runs[1][0]):
        for k in common.KEYS:
            assert a[k] == b[k], k
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k


@pytest.mark.parametrize("variant", ["momentum", "two_groups"])
def test_other_rmsprop_falls_back_to_torch(golden_dir, dev, variant):
    """RMSprop with momentum, or over two param groups, is not the update the flat pass
    computes: torch's optimiser steps it (nothing is bound), and the result matches the
    generic loop's on the same policy."""
    z = common.golden(golden_dir)

    def optim(params):
        kw = dict(lr=7e-4, eps=1e-5, alpha=0.99)
        if variant == "momentum":
            return torch.optim.RMSprop(params, momentum=0.9, **kw)
        return torch.optim.RMSprop([dict(params=params[:5]), dict(params=params[5:])], **kw)

    runs = []
    for generic in (False, True):
        policy, cfg = common.build_policy(z, "rms_multi", dev, optim=optim)
        batch = common.learn_batch(z, "rms_multi", dev)
        np.random.seed(21)
        learn = policy._learn_generic if generic else policy.learn
        res = learn(batch, cfg["batch_size"], cfg["repeat"])
        assert tuple(res) == common.KEYS
        assert not policy._mlp.adam_bound(policy.optim)
        key = "momentum_buffer" if variant == "momentum" else "square_avg"
        assert all(key in policy.optim.state[p] for p in policy._actor_critic.parameters())
        runs.append((res, {k: v.detach().cpu().numpy() for k, v in policy.state_dict().items()}))
    for k in common.KEYS:
        np.testing.assert_allclose(runs[0][0][k], runs[1][0][k], rtol=2e-5, atol=1e-6, err_msg=k)
    # the fused minibatch's gradients are within ~1e-6 relative of autograd's (typical |g|
    # 5e-3 after the 0.5 clip over 11 079 parameters: 5e-9 absolute); an RMSprop step moves by
    # at most lr / eps = 70 per unit of gradient, over 8 steps, times 1 / (1 - 0.9) with
    # momentum: 8 * 10 * 70 * 5e-9 = 2.8e-5, rounded up
    for k, a in runs[1][1].items():
        np.testing.assert_allclose(runs[0][1][k], a, rtol=1e-5, atol=1e-4, err_msg=k)



# -- masked and wide Categorical policies (tests/loss_edges_common.py) --------------------------
def test_learn_masked_actor_matches_generic(dev):
    """An actor that writes -inf over illegal actions, A2CPolicy.learn on the fused Categorical
    path against a twin with the same weights and seed on _learn_generic: every parameter
    finite, losses and parameters at tests/test_gpu_ppo_discrete.py's
    test_learn_discrete_matches_reference tolerances."""
    from tianshou_amd.policy import A2CPolicy
    from tests import loss_edges_common as lc
    policy, twin = lc.discrete_policy(A2CPolicy, dev, lambda: lc.MaskedActor(dev), 6, seed=41)
    assert policy._cat == 0 and not policy._fused
    batch = lc.discrete_batch(policy, dev, 200, 6, seed=42, illegal=lc.MASKED_ACTIONS)
    fused = lc.count_calls(policy, "_learn_cat")
    np.random.seed(21)
    res = policy.learn(batch, batch_size=64, repeat=2)
    assert fused == ["_learn_cat"]
    np.random.seed(21)
    res_twin = twin._learn_generic(batch, 64, 2)
    print("masked A2C losses:", res["loss"])
    lc.compare_runs(res, res_twin, lc.state_of(policy), lc.state_of(twin), common.KEYS,
                    (1e-4, 1e-5), (1e-5, 1e-6), "masked A2C")


@pytest.mark.parametrize("n_act", [65, 100])
def test_wide_categorical_policy(dev, n_act):
    """More actions than the loss kernels take: A2CPolicy's process_fn and learn() run the
    generic loop, bit for bit the twin's forced onto it."""
    from tianshou_amd.policy import A2CPolicy
    from tianshou_amd.utils.net import DiscreteActor, Net
    from tests import loss_edges_common as lc
    make = lambda: DiscreteActor(Net(8, hidden_sizes=(64, 64), device=dev), n_act,  # noqa: E731
                                 softmax_output=False, device=dev)
    policy, twin = lc.discrete_policy(A2CPolicy, dev, make, n_act, seed=43)
    runs = []
    for pol in (policy, twin):
        buf = lc.filled_buffer(dev, 8, 25, 8, lambda rng, E: rng.randint(0, n_act, E), seed=44)
        batch, idx = buf.sample(0)
        batch = pol.process_fn(batch, buf, idx)
        generic, fused = lc.count_calls(pol, "_learn_generic"), lc.count_calls(pol, "_learn_cat")
        np.random.seed(21)
        if pol is policy:
            res = pol.learn(batch, batch_size=64, repeat=2)
            assert (len(generic), len(fused)) == (1, 0)
        else:
            res = pol._learn_generic(batch, 64, 2)
        assert all(np.isfinite(res[k]).all() for k in res)
        runs.append((res, lc.state_of(pol)))
    assert runs[0][0] == runs[1][0]  # bit for bit
    for k, v in runs[0][1].items():
        assert torch.equal(v, runs[1][1][k]), k
