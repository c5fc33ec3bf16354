"""tests/golden/iqn.npz (tools/gen_goldens.py gen_iqn: the reference IQNPolicy over
ImplicitQuantileNetwork(Net(...)) on CPU torch) pinned on the host.

A torch-CPU restatement of iqn.py:62-112 and utils/net/discrete.py:124-214 replays every variant
from the recorded sample indices, importance weights and torch.rand draws; this package's
IQNPolicy on the CPU (``fused = False``) then runs the same updates from the recorded torch seed
alone and must draw the recorded fractions bit for bit, which pins the draw order and shapes.
tests/test_gpu_iqn.py compares the device policy with the same file.

Tolerances as tests/test_dist_dqn_host.py: n-step returns exact in f32, losses, outgoing
priorities and parameters rtol 1e-6."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref
from tests import test_dqn_host as dh
from tests.conftest import GOLDEN, ROOT
from tianshou_amd.policy import IQNPolicy  # fails before IQNPolicy existed: so does this file

SYMBOLS = ("tsrl_iqn_embed_fwd", "tsrl_iqn_embed_bwd", "tsrl_iqn_select", "tsrl_iqn_loss_fwd_bwd")
TAGS = ("target", "uneven", "notarget", "per", "rms")


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(GOLDEN, "iqn.npz"))


@pytest.fixture(scope="module")
def cfg(z):
    return json.loads(str(z["learn_cfg"]))


def init_state(z):
    return {k[len("init_"):]: torch.as_tensor(z[k]) for k in z.files if k.startswith("init_")}


def make_optim(v, params):
    if v["optim"] == "rms":
        return torch.optim.RMSprop(params, lr=7e-4, eps=1e-5, alpha=0.99)
    return torch.optim.Adam(params, lr=1e-3)


# -- the restatement -------------------------------------------------------------------------------
def mlp(P, prefix, x):
    """Linear (ReLU Linear)*: the layers ``prefix.0``, ``prefix.2``, ... of a reference MLP."""
    i = 0
    while f"{prefix}.{i}.weight" in P:
        if i:
            x = torch.relu(x)
        x = F.linear(x, P[f"{prefix}.{i}.weight"], P[f"{prefix}.{i}.bias"])
        i += 2
    return x


def iqn_forward(P, obs, taus):
    """discrete.py:143-155, 201-214 with the fractions handed in: [b, A, N]."""
    h = mlp(P, "preprocess.model.model", obs)
    b, N = taus.shape
    C = P["embed_model.net.0.weight"].shape[1]
    i_pi = np.pi * torch.arange(start=1, end=C + 1, dtype=taus.dtype).view(1, 1, C)
    cosines = torch.cos(taus.view(b, N, 1) * i_pi).view(b * N, C)
    emb = torch.relu(F.linear(cosines, P["embed_model.net.0.weight"],
                              P["embed_model.net.0.bias"])).view(b, N, -1)
    x = (h.unsqueeze(1) * emb).view(b * N, -1)
    return mlp(P, "last.model", x).view(b, N, -1).transpose(1, 2)


def top2_gap(q):
    q = np.sort(np.asarray(q, np.float64), axis=1)
    best, second = q[:, -1], q[:, -2]
    return float(((best - second) / np.maximum(np.abs(best), np.abs(second))).min())


def terminal_rows(vb, idx, n_step):
    terminal = idx % vb.maxsize
    for _ in range(n_step - 1):
        terminal = vb.next(terminal)
    return terminal


@pytest.mark.parametrize("tag", TAGS)
def test_variant_replays_from_recorded_indices_and_draws(z, cfg, tag):
    v = cfg["variants"][tag]
    vb, store = dh.host_buffer(z, cfg)
    np.testing.assert_array_equal(vb.sizes, z["buf_lengths"])
    np.testing.assert_array_equal(vb.last_index, z["buf_last_index"])
    P = {k: t.clone().requires_grad_(True) for k, t in init_state(z).items()}
    old = {k: t.detach().clone() for k, t in P.items()}
    optim = make_optim(v, list(P.values()))
    gaps = []
    for u in range(cfg["updates"]):
        q = f"{tag}_u{u}_"
        idx = z[q + "indices"]
        assert len(idx) == v["bs"]
        draws = [torch.as_tensor(z[q + f"draw{i}"]) for i in range(3 if v["freq"] else 2)]
        assert q + f"draw{len(draws)}" not in z.files
        assert all(0.0 <= float(d.min()) and float(d.max()) < 1.0 for d in draws)
        # process_fn: qrdqn.py:58-68 at the chain's last row, then the n-step return
        s_next = torch.as_tensor(store["obs_next"][terminal_rows(vb, idx, v["n_step"])])
        with torch.no_grad():
            sel = iqn_forward(P, s_next, draws[0])
            assert sel.shape == (v["bs"], cfg["A"], v["N"])
            gaps.append(top2_gap(sel.double().mean(2).numpy()))
            act = sel.mean(2).max(dim=1)[1]
            nxt = iqn_forward(old, s_next, draws[1]) if v["freq"] else sel
            tq = nxt[np.arange(len(act)), act, :]
        assert tq.shape == (v["bs"], v["M"] if v["freq"] else v["N"])
        returns, _ = ref.nstep_return(vb, store["terminated"], idx, tq.numpy(), cfg["gamma"],
                                      v["n_step"])
        assert returns.dtype == np.float32
        np.testing.assert_array_equal(returns, z[q + "returns"], err_msg=q)
        # learn: iqn.py:88-112
        if v["freq"] and u % v["freq"] == 0:
            old = {k: t.detach().clone() for k, t in P.items()}
        optim.zero_grad()
        w = torch.as_tensor(z[q + "weight"]) if v.get("per") else 1.0
        taus = draws[-1]
        curr = iqn_forward(P, torch.as_tensor(store["obs"][idx]), taus)
        curr = curr[np.arange(len(idx)), store["act"][idx], :].unsqueeze(2)
        target = torch.as_tensor(returns).unsqueeze(1)
        N, M = curr.shape[1], target.shape[2]
        diff = F.smooth_l1_loss(target.expand(-1, N, -1), curr.expand(-1, -1, M),
                                reduction="none")
        huber = (diff * (taus.unsqueeze(2) - (target - curr).detach().le(0.).float()).abs()) \
            .sum(-1).mean(1)
        loss = (huber * w).mean()
        loss.backward()
        optim.step()
        np.testing.assert_allclose(loss.item(), float(z[q + "loss"]), rtol=1e-6, err_msg=q)
        np.testing.assert_allclose(diff.detach().abs().sum(-1).mean(1).numpy(),
                                   z[q + "out_weight"], rtol=1e-6, atol=1e-6, err_msg=q)
        for k, t in P.items():
            np.testing.assert_allclose(t.detach().numpy(), z[q + "param_" + k], rtol=1e-6,
                                       atol=1e-9, err_msg=q + k)
    np.testing.assert_allclose(min(gaps), float(z[tag + "_top2_gap"]), rtol=1e-3)
    assert float(z[tag + "_top2_gap"]) >= 1e-6, tag


# -- this package's policy on the CPU --------------------------------------------------------------
def make_policy(z, cfg, tag, device="cpu"):
    from tianshou_amd.utils.net import ImplicitQuantileNetwork, Net
    v, n = cfg["variants"][tag], cfg["net"]
    feature = Net(cfg["D"], n["feature_out"], hidden_sizes=n["feature_hidden"], device=device)
    net = ImplicitQuantileNetwork(feature, cfg["A"], hidden_sizes=n["head_hidden"],
                                  num_cosines=n["num_cosines"], device=device).to(device)
    net.load_state_dict(init_state(z), strict=True)
    policy = IQNPolicy(net, make_optim(v, net.parameters()), discount_factor=cfg["gamma"],
                       sample_size=cfg["sample_size"], online_sample_size=v["N"],
                       target_sample_size=v["M"], estimation_step=v["n_step"],
                       target_update_freq=v["freq"]).to(device)
    return policy, v


@pytest.mark.parametrize("tag", TAGS)
def test_same_seed_draws_the_recorded_stream(z, cfg, tag):
    from tianshou_amd.data import Batch
    policy, v = make_policy(z, cfg, tag)
    assert policy.fused and policy.model.fused_embed
    policy.fused = False
    assert not policy.fused and not policy.model.fused_embed
    assert not v["freq"] or not policy.model_old.fused_embed
    policy.train()
    vb, store = dh.host_buffer(z, cfg)
    sample, drawn = policy._sample_taus, []

    def rec_taus(shape, device):
        drawn.append(sample(shape, device))
        return drawn[-1]

    policy._sample_taus = rec_taus
    torch.manual_seed(cfg["draw_seed"])
    for u in range(cfg["updates"]):
        q = f"{tag}_u{u}_"
        idx = z[q + "indices"]
        del drawn[:]
        s_next = torch.as_tensor(store["obs_next"][terminal_rows(vb, idx, v["n_step"])])
        tq = policy._next_rows(Batch(obs_next=s_next, info=Batch()))
        returns, _ = ref.nstep_return(vb, store["terminated"], idx, tq.numpy(), cfg["gamma"],
                                      v["n_step"])
        np.testing.assert_array_equal(returns, z[q + "returns"], err_msg=q)
        batch = Batch(obs=torch.as_tensor(store["obs"][idx]),
                      act=torch.as_tensor(store["act"][idx]),
                      obs_next=torch.as_tensor(store["obs_next"][idx]),
                      returns=torch.as_tensor(returns), info=Batch())
        if v.get("per"):
            batch.weight = torch.as_tensor(z[q + "weight"])
        res = policy.learn(batch)
        assert len(drawn) == (3 if v["freq"] else 2)
        for i, d in enumerate(drawn):
            assert d.dtype == torch.float32
            np.testing.assert_array_equal(d.numpy(), z[q + f"draw{i}"], err_msg=f"{q}draw{i}")
        np.testing.assert_allclose(res["loss"], float(z[q + "loss"]), rtol=1e-6, err_msg=q)
        np.testing.assert_allclose(batch.weight.numpy(), z[q + "out_weight"], rtol=1e-6,
                                   atol=1e-6, err_msg=q)
        for k, t in policy.model.state_dict().items():
            np.testing.assert_allclose(t.numpy(), z[q + "param_" + k], rtol=1e-6, atol=1e-9,
                                       err_msg=q + k)
    assert policy._iter == cfg["updates"] and policy._flat is None


def test_network_draws_its_own_fractions_when_none_are_given(z, cfg):
    """forward(obs, sample_size) alone is the reference's: one torch.rand after the preprocess
    forward, and ((out, taus), hidden) with out the [b, A, N] view of [b, N, A]."""
    policy, _ = make_policy(z, cfg, "target")
    net = policy.model
    obs = torch.as_tensor(z["add_obs"][:5])
    torch.manual_seed(3)
    (out, taus), hidden = net(obs, sample_size=7)
    torch.manual_seed(3)
    want = torch.rand(5, 7)
    assert torch.equal(taus, want) and hidden is None
    assert out.shape == (5, cfg["A"], 7) and out.transpose(1, 2).is_contiguous()
    (again, t2), _ = net(obs, sample_size=7, taus=want)
    assert t2 is want and torch.equal(again, out)
    P = {k: t for k, t in net.state_dict().items()}
    torch.testing.assert_close(out, iqn_forward(P, obs, want), rtol=1e-6, atol=1e-7)


def test_state_dict_keys_are_the_references(z, cfg):
    policy, _ = make_policy(z, cfg, "target")
    keys = list(policy.model.state_dict())
    assert keys == json.loads(str(z["state_keys"]))
    assert all(k.startswith(("preprocess.", "last.", "embed_model.net.0.")) for k in keys)
    assert {"embed_model.net.0.weight", "embed_model.net.0.bias"} <= set(keys)


def test_constructor_arguments_and_assertions():
    from tianshou_amd.policy import DQNPolicy, QRDQNPolicy
    net = torch.nn.Linear(1, 1)
    p = IQNPolicy(net, None)
    assert isinstance(p, QRDQNPolicy) and isinstance(p, DQNPolicy)
    assert (p._sample_size, p._online_sample_size, p._target_sample_size) == (32, 8, 8)
    assert p._num_quantiles == 32 and tuple(p.tau_hat.shape) == (1, 32, 1)
    assert p._gamma == 0.99 and p._n_step == 1 and not p._target
    assert p.eager_collect_step and p.graph_learn is None and p.fused_adam
    p = IQNPolicy(net, None, 0.9, 16, 5, 7, 3, 4)
    assert (p._gamma, p._sample_size, p._online_sample_size, p._target_sample_size, p._n_step,
            p._freq) == (0.9, 16, 5, 7, 3, 4) and p._target
    for kw in (dict(sample_size=1), dict(online_sample_size=1), dict(target_sample_size=1)):
        with pytest.raises(AssertionError):
            IQNPolicy(net, None, **kw)
    # iqn.py:70-75: which network and which mode decide the sample size
    assert p._size_of("model_old") == 7 and p._size_of("model") == 5
    p.eval()
    assert p._size_of("model") == 16 and p._size_of("model_old") == 7
    # the loss kernel's column limit sends learn() to the torch formulation
    from tianshou_amd import _C
    wide = IQNPolicy(net, None, online_sample_size=_C.DIST_MAX_N + 1)
    assert wide._num_columns() == _C.DIST_MAX_N + 1 and not wide._fused_learn()
    # M counts only with a target network
    assert IQNPolicy(net, None, target_sample_size=_C.DIST_MAX_N + 1)._num_columns() == 8
    assert IQNPolicy(net, None, target_sample_size=_C.DIST_MAX_N + 1,
                     target_update_freq=1)._num_columns() == _C.DIST_MAX_N + 1


def test_foreign_network_is_never_handed_fractions():
    """A network that is not this package's ImplicitQuantileNetwork draws inside its forward;
    the policy passes no ``taus=`` and never captures it."""
    calls = []

    class Foreign(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(3, 2)

        def forward(self, obs, sample_size, **kwargs):
            calls.append((sample_size, sorted(kwargs)))
            taus = torch.rand(len(obs), sample_size)
            return (self.lin(obs).unsqueeze(2) * taus.unsqueeze(1), taus), None

    from tianshou_amd.data import Batch
    net = Foreign()
    policy = IQNPolicy(net, torch.optim.Adam(net.parameters(), lr=1e-3), online_sample_size=4,
                       target_sample_size=6, target_update_freq=2)
    policy._sample_taus = None  # any call would raise
    policy.train()
    obs = torch.randn(5, 3)
    res = policy(Batch(obs=obs, info=Batch()))
    assert res.logits.shape == (5, 2, 4) and res.taus.shape == (5, 4) and res.act.shape == (5,)
    rows = policy._next_rows(Batch(obs_next=obs, info=Batch()))
    assert rows.shape == (5, 6)
    assert calls == [(4, ["info", "state"]), (4, ["info", "state"]), (6, ["info", "state"])]
    assert policy._learn_inputs(Batch(returns=rows)) == ()
    assert not policy._graph_ok(obs, 5)
    loss = policy.learn(Batch(obs=obs, act=torch.zeros(5, dtype=torch.int64), returns=rows,
                              info=Batch()))["loss"]
    assert np.isfinite(loss)


def test_new_symbols_are_declared_and_bound():
    from tianshou_amd import _C
    from tianshou_amd import policy as pol
    from tianshou_amd.utils import net
    with open(os.path.join(ROOT, "include", "tsrl.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert name in _C.EXPORTED
        assert f" {name}(" in header
    assert f"#define TSRL_IQN_MAX_COSINES {_C.IQN_MAX_COSINES}\n" in header
    assert "IQNPolicy" in pol.__all__
    assert issubclass(net.ImplicitQuantileNetwork, net.DiscreteCritic)
    assert net.CosineEmbeddingNetwork(3, 5).net[0].weight.shape == (5, 3)


def test_select_cases_exclude_at_most_one_percent_of_rows():
    """tests/test_gpu_iqn.py compares tsrl_iqn_select's action with the f64 argmax on the rows
    whose f64 top-two relative gap is >= 1e-6: with its seeds the f64 reference alone leaves out
    at most 1 % of the rows of any case."""
    from tests import test_gpu_iqn as g
    for b in g.SEL_BS:
        for A in g.SEL_AS:
            for N, M in g.SEL_NM:
                sel, _ = g.select_inputs(b, A, N, M)
                gap = g.top2_rel_gap(sel.double().mean(2))
                out = int((gap < 1e-6).sum())
                assert out <= b // 100, (b, A, N, M, out)
