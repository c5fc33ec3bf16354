"""tests/golden/fqf.npz (tools/gen_goldens.py gen_fqf: the reference FQFPolicy over
FullQuantileFunction(Net(...)) and FractionProposalNetwork on CPU torch) pinned on the host.

This package's FQFPolicy on the CPU replays every variant from the recorded sample indices and
importance weights (an update has no random input): n-step returns exact in f32, the four losses
rtol 2e-5, outgoing priorities rtol 1e-6, the parameters of both networks rtol 1e-5 / atol 1e-6.
tests/test_gpu_fqf.py compares the device policy with the same file, and takes its f64 references
from the restatements below: ``propose_reference`` (discrete.py:241-249), ``gradient_of_taus``
(fqf.py:147-160) and ``g_logits_formula``, the analytic gradient documented in include/tsrl.h,
which is anchored here against torch.autograd on the reference lines."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref
from tests import test_dqn_host as dh
from tests.conftest import GOLDEN, ROOT
from tests.test_iqn_host import terminal_rows
from tianshou_amd.policy import FQFPolicy  # fails before FQFPolicy existed: so does this file

SYMBOLS = ("tsrl_fqf_propose_fwd", "tsrl_fqf_select", "tsrl_fqf_fraction_loss_fwd_bwd")
TAGS = ("target", "notarget", "uneven", "per", "rms")
LOSS_KEYS = ("loss", "loss/quantile", "loss/fraction", "loss/entropy")


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(GOLDEN, "fqf.npz"))


@pytest.fixture(scope="module")
def cfg(z):
    return json.loads(str(z["learn_cfg"]))


# -- restatements ----------------------------------------------------------------------------------
def propose_reference(logits):
    """discrete.py:241-249 from the proposal logits, in their dtype, without Categorical's
    argument check: (taus, tau_hats, entropies, logp)."""
    logp = logits - logits.logsumexp(dim=-1, keepdim=True)
    probs = F.softmax(logp, dim=-1)
    taus = F.pad(torch.cumsum(probs, dim=1), (1, 0))
    tau_hats = (taus[:, :-1] + taus[:, 1:]).detach() / 2.0
    entropies = -(torch.clamp(logp, min=torch.finfo(logp.dtype).min) * probs).sum(-1)
    return taus, tau_hats, entropies, logp


def gradient_of_taus(sa_quantile_hats, sa_quantiles):
    """fqf.py:147-160 in the inputs' dtype."""
    values_1 = sa_quantiles - sa_quantile_hats[:, :-1]
    signs_1 = sa_quantiles > torch.cat([sa_quantile_hats[:, :1], sa_quantiles[:, :-1]], dim=1)
    values_2 = sa_quantiles - sa_quantile_hats[:, 1:]
    signs_2 = sa_quantiles < torch.cat([sa_quantiles[:, 1:], sa_quantile_hats[:, -1:]], dim=1)
    return torch.where(signs_1, values_1, -values_1) + torch.where(signs_2, values_2, -values_2)


def g_logits_formula(G, logp, entropies, ent_coef):
    """The gradient of fraction_loss - ent_coef * entropy_loss towards the proposal logits, as
    tsrl_fqf_fraction_loss_fwd_bwd documents it, in f64: G [b, N - 1], logp [b, N], H [b]."""
    G, logp, H = G.double(), logp.double(), entropies.double().unsqueeze(1)
    b = G.shape[0]
    S = torch.cat([G.flip(1).cumsum(1).flip(1), torch.zeros(b, 1, dtype=torch.float64,
                                                            device=G.device)], dim=1) / b
    p = logp.exp()
    g = p * (S - (p * S).sum(1, keepdim=True)) + (ent_coef / b) * p * (logp + H)
    return torch.where(p == 0, torch.zeros_like(g), g)


@pytest.mark.parametrize("N", (2, 3, 8))
@pytest.mark.parametrize("ent_coef", (0.0, 10.0))
def test_analytic_logit_gradient_matches_autograd(N, ent_coef):
    g = torch.Generator().manual_seed(7 * N)
    b = 5
    logits = (2.0 * torch.randn(b, N, generator=g, dtype=torch.float64)).requires_grad_(True)
    hats = torch.randn(b, N, generator=g, dtype=torch.float64)
    quantiles = torch.randn(b, N - 1, generator=g, dtype=torch.float64)
    taus, _, entropies, logp = propose_reference(logits)
    G = gradient_of_taus(hats, quantiles)
    loss = (G * taus[:, 1:-1]).sum(1).mean() - ent_coef * entropies.mean()
    (want,) = torch.autograd.grad(loss, logits)
    got = g_logits_formula(G, logp.detach(), entropies.detach(), ent_coef)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-15)
    assert float(want.abs().max()) > 0


# -- this package's policy on the CPU --------------------------------------------------------------
def init_state(z, prefix="init_"):
    return {k[len(prefix):]: torch.as_tensor(z[k]) for k in z.files if k.startswith(prefix)}


def make_optims(v, cfg, net, propose):
    if v["optim"] == "rms":
        return (torch.optim.RMSprop(net.parameters(), lr=7e-4, eps=1e-5, alpha=0.99),
                torch.optim.RMSprop(propose.parameters(), lr=7e-4, eps=1e-5, alpha=0.99))
    return (torch.optim.Adam(net.parameters(), lr=1e-3),
            torch.optim.Adam(propose.parameters(), lr=cfg["fraction_lr"]))


def make_policy(z, cfg, tag, device="cpu", **attrs):
    from tianshou_amd.utils.net import FractionProposalNetwork, FullQuantileFunction, Net
    v, n = cfg["variants"][tag], cfg["net"]
    feature = Net(cfg["D"], n["feature_out"], hidden_sizes=n["feature_hidden"], device=device)
    net = FullQuantileFunction(feature, cfg["A"], hidden_sizes=n["head_hidden"],
                               num_cosines=n["num_cosines"], device=device).to(device)
    net.load_state_dict(init_state(z), strict=True)
    propose = FractionProposalNetwork(v["N"], net.input_dim).to(device)
    propose.load_state_dict(init_state(z, tag + "_pinit_"), strict=True)
    optim, frac_optim = make_optims(v, cfg, net, propose)
    policy = FQFPolicy(net, optim, propose, frac_optim, discount_factor=cfg["gamma"],
                       num_fractions=v["N"], ent_coef=v["ent_coef"],
                       estimation_step=v["n_step"], target_update_freq=v["freq"]).to(device)
    for k, a in attrs.items():
        setattr(policy, k, a)
    policy.train()
    return policy, v


@pytest.mark.parametrize("tag", TAGS)
def test_variant_replays_from_recorded_indices(z, cfg, tag):
    from tianshou_amd.data import Batch
    policy, v = make_policy(z, cfg, tag)
    assert policy._ent_coef == v["ent_coef"]
    vb, store = dh.host_buffer(z, cfg)
    np.testing.assert_array_equal(vb.sizes, z["buf_lengths"])
    np.testing.assert_array_equal(vb.last_index, z["buf_last_index"])
    for u in range(cfg["updates"]):
        q = f"{tag}_u{u}_"
        idx = z[q + "indices"]
        assert len(idx) == v["bs"]
        s_next = torch.as_tensor(store["obs_next"][terminal_rows(vb, idx, v["n_step"])])
        tq = policy._next_rows(Batch(obs_next=s_next, info=Batch()))
        assert tq.shape == (v["bs"], v["N"])
        returns, _ = ref.nstep_return(vb, store["terminated"], idx, tq.numpy(), cfg["gamma"],
                                      v["n_step"])
        assert returns.dtype == np.float32
        np.testing.assert_array_equal(returns, z[q + "returns"], err_msg=q)
        batch = Batch(obs=torch.as_tensor(store["obs"][idx]),
                      act=torch.as_tensor(store["act"][idx]),
                      obs_next=torch.as_tensor(store["obs_next"][idx]),
                      returns=torch.as_tensor(returns), info=Batch())
        if v.get("per"):
            batch.weight = torch.as_tensor(z[q + "weight"])
        res = policy.learn(batch)
        assert tuple(res) == LOSS_KEYS
        for k in LOSS_KEYS:
            np.testing.assert_allclose(res[k], float(z[q + k.replace("/", "_")]), rtol=2e-5,
                                       err_msg=q + k)
        np.testing.assert_allclose(batch.weight.numpy(), z[q + "out_weight"], rtol=1e-6,
                                   atol=1e-6, err_msg=q)
        assert not batch.weight.requires_grad
        for prefix, module in (("param_", policy.model), ("pparam_", policy.propose_model)):
            for k, t in module.state_dict().items():
                np.testing.assert_allclose(t.numpy(), z[q + prefix + k], rtol=1e-5, atol=1e-6,
                                           err_msg=q + prefix + k)
    assert policy._iter == cfg["updates"] and policy._flat is None and policy._frac_flat is None
    assert float(z[tag + "_top2_gap"]) >= 1e-6 and float(z[tag + "_min_margin"]) >= 1e-5
    # the proposal network moved visibly
    moved = np.abs(z[f"{tag}_u{cfg['updates'] - 1}_pparam_net.weight"]
                   - z[tag + "_pinit_net.weight"]).max()
    assert moved > 1e-4, moved


def test_recorded_margin_is_the_recordings_own(z, cfg):
    """min_margin restated from the recorded sa_quantile_hats / sa_quantiles."""
    for tag in TAGS:
        margins = []
        for u in range(cfg["updates"]):
            hats = z[f"{tag}_u{u}_sa_quantile_hats"].astype(np.float64)
            q = z[f"{tag}_u{u}_sa_quantiles"].astype(np.float64)
            assert hats.shape == (cfg["variants"][tag]["bs"], cfg["variants"][tag]["N"])
            assert q.shape == (hats.shape[0], hats.shape[1] - 1)
            left = np.concatenate([hats[:, :1], q[:, :-1]], axis=1)
            right = np.concatenate([q[:, 1:], hats[:, -1:]], axis=1)
            margins.append(min(np.abs(q - left).min(), np.abs(q - right).min()))
        assert min(margins) == float(z[tag + "_min_margin"]) >= 1e-5


@pytest.mark.parametrize("N", (5, 8))
def test_seeded_construction_reproduces_the_recorded_proposal_weights(z, cfg, N):
    from tianshou_amd.utils.net import FractionProposalNetwork
    tag = "uneven" if N == 5 else "target"
    assert cfg["variants"][tag]["N"] == N
    torch.manual_seed(cfg["init_seed"] + N)
    net = FractionProposalNetwork(N, cfg["net"]["feature_out"])
    assert (net.num_fractions, net.embedding_dim) == (N, cfg["net"]["feature_out"])
    np.testing.assert_array_equal(net.net.weight.detach().numpy(), z[tag + "_pinit_net.weight"])
    np.testing.assert_array_equal(net.net.bias.detach().numpy(), z[tag + "_pinit_net.bias"])
    assert float(net.net.bias.detach().abs().max()) == 0.0


def test_state_dict_keys_are_the_references(z, cfg):
    policy, _ = make_policy(z, cfg, "target")
    keys = list(policy.model.state_dict())
    assert keys == json.loads(str(z["state_keys"]))
    assert all(k.startswith(("preprocess.", "last.", "embed_model.net.0.")) for k in keys)
    assert list(policy.propose_model.state_dict()) == json.loads(str(z["propose_keys"])) == \
        ["net.weight", "net.bias"]


def test_network_forward_follows_the_reference(z, cfg):
    from tianshou_amd.data import Batch
    policy, v = make_policy(z, cfg, "target")
    net, propose = policy.model, policy.propose_model
    obs = torch.as_tensor(z["add_obs"][:5])
    (quantiles, fractions, quantiles_tau), hidden = net(obs, propose_model=propose)
    assert hidden is None and isinstance(fractions, Batch)
    assert quantiles.shape == (5, cfg["A"], v["N"]) and quantiles_tau.shape == \
        (5, cfg["A"], v["N"] - 1) and not quantiles_tau.requires_grad
    h, _ = net.preprocess(obs)
    want = propose_reference(propose.net(h.detach()))
    for got, w in zip((fractions.taus, fractions.tau_hats, fractions.entropies), want):
        torch.testing.assert_close(got, w, rtol=1e-6, atol=1e-7)
    assert fractions.taus.requires_grad and not fractions.tau_hats.requires_grad
    assert torch.equal(quantiles_tau, net._compute_quantiles(h, fractions.taus[:, 1:-1]))
    # handed-in fractions are used as they are; no second pass where nobody reads it, or in eval
    (again, same, _), _ = net(obs, propose_model=None, fractions=fractions)
    assert same is fractions and torch.equal(again, quantiles)
    assert net(obs, propose_model=propose, want_quantiles_tau=False)[0][2] is None
    net.eval()
    assert net(obs, propose_model=propose)[0][2] is None


def test_constructor_arguments_and_attributes():
    from tianshou_amd import _C
    from tianshou_amd.policy import DQNPolicy, QRDQNPolicy
    net, frac = torch.nn.Linear(1, 1), torch.nn.Linear(1, 1)
    opt, fopt = object(), object()
    p = FQFPolicy(net, opt, frac, fopt)
    assert isinstance(p, QRDQNPolicy) and isinstance(p, DQNPolicy)
    assert p.model is net and p.optim is opt and p.propose_model is frac
    assert p._fraction_optim is fopt and p._ent_coef == 0.0 and p._num_quantiles == 32
    assert p._gamma == 0.99 and p._n_step == 1 and not p._target and not p._rew_norm
    assert not getattr(p, "eager_collect_step", False) and p.graph_learn is None and p.fused_adam
    p = FQFPolicy(net, opt, frac, fopt, 0.9, 16, 0.5, 3, 4, True)
    assert (p._gamma, p._num_quantiles, p._ent_coef, p._n_step, p._freq, p._rew_norm) == \
        (0.9, 16, 0.5, 3, 4, True) and p._target
    with pytest.raises(AssertionError):
        FQFPolicy(net, opt, frac, fopt, num_fractions=1)
    # the kernels' width limit sends learn() to the torch formulation
    wide = FQFPolicy(net, opt, frac, fopt, num_fractions=_C.DIST_MAX_N + 1)
    assert wide._num_columns() == _C.DIST_MAX_N + 1 and not wide._fused_learn()


def test_fused_switch_reaches_every_network(z, cfg):
    policy, _ = make_policy(z, cfg, "target")
    nets = (policy.model, policy.model_old)
    assert policy.fused and policy.propose_model.fused and all(n.fused_embed for n in nets)
    policy.fused = False
    assert not policy.propose_model.fused and not any(n.fused_embed for n in nets)
    policy.fused = True
    assert policy.propose_model.fused and all(n.fused_embed for n in nets)


def test_sync_weight_leaves_the_proposal_network_alone(z, cfg):
    policy, _ = make_policy(z, cfg, "target")
    before = {k: t.clone() for k, t in policy.propose_model.state_dict().items()}
    with torch.no_grad():
        for p in policy.model.parameters():
            p.add_(1.0)
    assert not hasattr(policy, "propose_model_old")
    assert not any(p is q for p in policy.model_old.parameters()
                   for q in policy.propose_model.parameters())
    policy.sync_weight()
    for (k, a), b in zip(policy.model.state_dict().items(),
                         policy.model_old.state_dict().values()):
        assert torch.equal(a, b), k
    for k, t in policy.propose_model.state_dict().items():
        assert torch.equal(t, before[k])


def test_foreign_networks_are_never_captured():
    """A model that is not this package's FullQuantileFunction (or a fraction_model that is not
    its FractionProposalNetwork) is called as the reference calls it and never captured."""
    from tianshou_amd.data import Batch
    from tianshou_amd.utils.net import FractionProposalNetwork
    calls = []

    class Foreign(torch.nn.Module):
        training_only = True

        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(3, 2 * 4)

        def forward(self, obs, propose_model, fractions=None, **kwargs):
            calls.append(sorted(kwargs))
            if fractions is None:
                taus, tau_hats, ent = propose_model(obs.detach())
                fractions = Batch(taus=taus, tau_hats=tau_hats, entropies=ent)
            base = self.lin(obs).view(-1, 2, 4)
            q = base + fractions.tau_hats.unsqueeze(1)
            q_tau = (base[:, :, :-1] + fractions.taus[:, 1:-1].unsqueeze(1)).detach()
            return (q, fractions, q_tau), None

    net, frac = Foreign(), FractionProposalNetwork(4, 3)
    policy = FQFPolicy(net, torch.optim.Adam(net.parameters(), lr=1e-3), frac,
                       torch.optim.Adam(frac.parameters(), lr=1e-3), num_fractions=4,
                       ent_coef=1.0, target_update_freq=2)
    policy.train()
    obs = torch.randn(5, 3)
    assert not policy._own_nets() and not policy._graph_ok(obs, 5)
    res = policy(Batch(obs=obs, info=Batch()))
    assert res.logits.shape == (5, 2, 4) and res.fractions.taus.shape == (5, 5)
    assert res.act.shape == (5,) and res.quantiles_tau.shape == (5, 2, 3)
    rows = policy._next_rows(Batch(obs_next=obs, info=Batch()))
    assert rows.shape == (5, 4)
    assert calls == [["info", "state"]] * 3  # never handed want_quantiles_tau
    before = frac.net.weight.detach().clone()
    out = policy.learn(Batch(obs=obs, act=torch.zeros(5, dtype=torch.int64), returns=rows,
                             info=Batch()))
    assert tuple(out) == LOSS_KEYS and all(np.isfinite(list(out.values())))
    assert not torch.equal(frac.net.weight.detach(), before)
    # this package's quantile network with a foreign proposal network is foreign too
    own, _ = make_policy(np.load(os.path.join(GOLDEN, "fqf.npz")),
                         json.loads(str(np.load(os.path.join(GOLDEN, "fqf.npz"))["learn_cfg"])),
                         "target")
    assert own._own_nets()
    own.propose_model = torch.nn.Linear(16, 8)
    assert not own._own_nets() and not own._graph_ok(obs, 5)


def test_new_symbols_are_declared_and_bound():
    from tianshou_amd import _C
    from tianshou_amd import policy as pol
    from tianshou_amd.utils import net
    with open(os.path.join(ROOT, "include", "tsrl.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert name in _C.EXPORTED
        assert f" {name}(" in header
    # the width guards of FractionProposalNetwork / FQFPolicy read these
    assert f"#define TSRL_DIST_MAX_N {_C.DIST_MAX_N}\n" in header
    assert f"#define TSRL_IQN_MAX_COSINES {_C.IQN_MAX_COSINES}\n" in header
    assert "FQFPolicy" in pol.__all__
    assert issubclass(net.FullQuantileFunction, net.ImplicitQuantileNetwork)
    wide = net.FractionProposalNetwork(_C.DIST_MAX_N + 1, 2)
    assert not wide.takes_kernel(torch.zeros(1, 2))  # and a CPU tensor never does


def test_select_cases_exclude_at_most_one_percent_of_rows():
    """tests/test_gpu_fqf.py compares tsrl_fqf_select's action with the f64 argmax on the rows
    whose f64 top-two relative gap is >= 1e-6: with its seeds the f64 reference alone leaves out
    at most 1 % of the rows of any case."""
    from tests import test_gpu_fqf as g
    for b in g.SEL_BS:
        for A in g.SEL_AS:
            for N in g.SEL_NS:
                sel, _, taus = g.select_inputs(b, A, N)
                gap = g.top2_rel_gap(g.weighted_q64(sel, taus))
                out = int((gap < 1e-6).sum())
                assert out <= b // 100, (b, A, N, out)


def test_fraction_loss_cases_hold_exact_ties_of_each_kind():
    """The dyadic inputs of tests/test_gpu_fqf.py's fraction-loss cases hold ties of both sign
    tests (q_i == L_i and q_i == R_i) wherever N > 2 leaves room for them."""
    from tests import test_gpu_fqf as g
    for b in g.SEL_BS[1:]:
        for N in g.FRAC_NS:
            curr, qtau, act = g.fraction_inputs(b, 6, N)
            rows = torch.arange(b)
            left, right = g.tie_counts(curr[rows, act], qtau[rows, act])
            assert left > 0 and right > 0, (b, N, left, right)
