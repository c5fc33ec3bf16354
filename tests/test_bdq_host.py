"""tests/golden/bdq.npz (tools/gen_goldens.py gen_bdq: the reference BranchingDQNPolicy over
BranchingNet on CPU torch, and its ContinuousToDiscrete wrapper) pinned on the host.

This package's BranchingDQNPolicy on the CPU (``fused`` has nothing to fuse there: the torch
formulation runs) replays every variant from the recorded sample indices and importance weights:
returns rtol 1e-5 / atol 1e-6 (the reference rounds the branch mean and gamma * mean to f32, this
package computes the target in f64 and rounds once), losses rtol 2e-5 / atol 1e-6, outgoing
weights rtol 1e-4, parameters rtol 1e-5 / atol 1e-6 -- the bounds tests/test_gpu_bdq.py holds the
device policy to against the same file.  ``f64_forward`` and ``td_reference`` are the f64
restatements both files use."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import ref
from tests.conftest import GOLDEN, ROOT
from tianshou_amd.policy import BranchingDQNPolicy  # fails before the policy existed

SYMBOLS = ("tsrl_bdq_combine_fwd", "tsrl_bdq_combine_bwd", "tsrl_bdq_target",
           "tsrl_bdq_td_fwd_bwd")
TAGS = ("double_target", "nature", "notarget", "per", "rms", "one_branch")


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(GOLDEN, "bdq.npz"))


@pytest.fixture(scope="module")
def cfg(z):
    return json.loads(str(z["learn_cfg"]))


# -- restatements ----------------------------------------------------------------------------------
def top2_gap(q):
    """min over rows of (best - second) / max(|best|, |second|), f64 (the generator's)."""
    q = np.sort(np.asarray(q, np.float64), axis=1)
    if q.shape[1] < 2:
        return np.inf
    best, second = q[:, -1], q[:, -2]
    return float(((best - second) / np.maximum(np.abs(best), np.abs(second))).min())


def f64_forward(sd, obs, K):
    """common.py:535-543 in f64 from a state_dict of f32 arrays."""
    sd = {k: np.asarray(v, np.float64) for k, v in sd.items()}

    def mlp(prefix, x):
        n = 1 + max(int(k[len(prefix):].split(".")[0]) for k in sd if k.startswith(prefix))
        for i in range(0, n, 2):
            x = x @ sd[f"{prefix}{i}.weight"].T + sd[f"{prefix}{i}.bias"]
            if i + 1 < n:
                x = np.maximum(x, 0.0)
        return x

    h = np.maximum(mlp("common.model.", np.asarray(obs, np.float64)), 0.0)
    v = mlp("value.model.", h)
    s = np.stack([mlp(f"branches.{k}.model.", h) for k in range(K)], 1)
    return v[:, None, :] + s - s.mean(2, keepdims=True)


def td_reference(q, act, returns, weight):
    """bdq.py:115-124 in f64: (loss, prio [b], grad_q [b, K, A])."""
    q = np.asarray(q, np.float64)
    b, K, A = q.shape
    qa = np.take_along_axis(q, act[..., None], 2)[..., 0]
    td = np.asarray(returns, np.float64)[:, None] - qa
    w = np.ones(b) if weight is None else np.asarray(weight, np.float64)
    loss = ((td ** 2).mean(1) * w).mean()
    grad = np.zeros_like(q)
    np.put_along_axis(grad, act[..., None], (-2.0 * td * w[:, None] / (b * K))[..., None], 2)
    return loss, td.sum(1), grad


# -- the recorded stream ------------------------------------------------------------------------------
def host_buffer(z, cfg, tag):
    """The recorded add() stream through oracle.ref.VecBufferIndex, with the variant's [k, K]
    actions."""
    K = cfg["variants"][tag]["K"]
    vb = ref.VecBufferIndex(cfg["E"] * cfg["S"], cfg["E"])
    store = dict(obs=np.zeros((vb.maxsize, cfg["D"]), np.float32),
                 obs_next=np.zeros((vb.maxsize, cfg["D"]), np.float32),
                 act=np.zeros((vb.maxsize, K), np.int64), rew=np.zeros(vb.maxsize),
                 terminated=np.zeros(vb.maxsize, bool), truncated=np.zeros(vb.maxsize, bool))
    o = 0
    for k in z["add_len"]:
        sl = slice(o, o + int(k))
        row = {key: z["add_" + key][sl] for key in ("obs", "rew", "terminated", "truncated",
                                                    "obs_next")}
        row["act"] = z[tag + "_add_act"][sl]
        ptr, *_ = vb.add(row["rew"], row["terminated"], row["truncated"], z["add_ids"][sl])
        for key in store:
            store[key][ptr] = row[key]
        o += int(k)
    return vb, store


def init_state(z, prefix):
    return {k[len(prefix):]: torch.as_tensor(z[k]) for k in z.files if k.startswith(prefix)}


def make_net(cfg, v, device="cpu"):
    from tianshou_amd.utils.net import BranchingNet
    n = cfg["net"]
    return BranchingNet(cfg["D"], v["K"], v["A"], n["common"], n["value"], n["action"],
                        device=device)


def make_policy(z, cfg, tag, device="cpu", **attrs):
    v = cfg["variants"][tag]
    net = make_net(cfg, v, device).to(device)
    net.load_state_dict(init_state(z, tag + "_init_"), strict=True)
    if v["optim"] == "rms":
        optim = torch.optim.RMSprop(net.parameters(), lr=7e-4, eps=1e-5, alpha=0.99)
    else:
        optim = torch.optim.Adam(net.parameters(), lr=1e-3, eps=cfg["adam_eps"])
    policy = BranchingDQNPolicy(net, optim, discount_factor=cfg["gamma"], estimation_step=1,
                                target_update_freq=v["freq"], is_double=v["is_double"]).to(device)
    for k, a in attrs.items():
        setattr(policy, k, a)
    policy.train()
    return policy, v


def flat(module):
    return np.concatenate([t.detach().cpu().numpy().ravel() for t in module.parameters()])


def end_flags(vb, store, idx):
    done = store["terminated"] | store["truncated"]
    return done[idx] | np.isin(idx, vb.unfinished_index())


# -- the policy on the CPU ---------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_variant_replays_from_recorded_indices(z, cfg, tag):
    from tianshou_amd.data import Batch
    policy, v = make_policy(z, cfg, tag, fused=False)
    vb, store = host_buffer(z, cfg, tag)
    K, A = v["K"], v["A"]
    for u in range(cfg["updates"]):
        q = f"{tag}_"
        idx = z[q + "indices"][u]
        assert len(idx) == v["bs"]
        ret = policy._target_return(torch.as_tensor(store["obs_next"][idx]), store["rew"][idx],
                                    end_flags(vb, store, idx))
        assert ret.shape == (v["bs"],) and ret.dtype == torch.float32
        np.testing.assert_allclose(ret.numpy(), z[q + "returns"][u], rtol=1e-5, atol=1e-6,
                                   err_msg=f"{q}{u}")
        batch = Batch(obs=torch.as_tensor(store["obs"][idx]),
                      act=torch.as_tensor(store["act"][idx]),
                      returns=ret[:, None, None].expand(len(idx), K, A), info=Batch())
        if v.get("per"):
            batch.weight = torch.as_tensor(z[q + "weight"][u])
        res = policy.learn(batch)
        assert tuple(res) == ("loss",)
        np.testing.assert_allclose(res["loss"], float(z[q + "loss"][u]), rtol=2e-5, atol=1e-6)
        np.testing.assert_allclose(batch.weight.numpy(), z[q + "td_error"][u], rtol=1e-4)
        assert not batch.weight.requires_grad and batch.weight.shape == (v["bs"],)
        np.testing.assert_allclose(flat(policy.model), z[q + "params"][u], rtol=1e-5, atol=1e-6)
        if v["freq"] > 0:
            np.testing.assert_allclose(flat(policy.model_old), z[q + "params_old"][u],
                                       rtol=1e-5, atol=1e-6)
    assert policy._iter == cfg["updates"] and policy._flat is None


@pytest.mark.parametrize("tag", TAGS)
def test_recording_conditions_hold_in_the_file(z, cfg, tag):
    """The three conditions the generator asserts, recomputed from the recorded arrays: the
    sampled rows hold each kind of episode end, every per-branch top-two gap of the selecting
    network is >= 1e-4 (f64 forward from the recorded parameters), every |sum_k td| >= 1e-2."""
    v, chk = cfg["variants"][tag], cfg["checks"][tag]
    vb, store = host_buffer(z, cfg, tag)
    idx = z[tag + "_indices"]
    assert ((store["truncated"] & ~store["terminated"])[idx]).sum() == chk["trunc"] > 0
    assert store["terminated"][idx].sum() == chk["term"] > 0
    assert np.isin(idx, vb.unfinished_index()).sum() == chk["unfinished"] > 0
    min_td = float(np.abs(z[tag + "_td_error"]).min())
    assert min_td == pytest.approx(chk["min_td"]) and min_td >= cfg["min_td"]
    # the selecting network at update u: the online one (double, or no target) before the
    # update, else the target as last synced
    names = list(init_state(z, tag + "_init_"))
    shapes = [tuple(z[f"{tag}_init_{k}"].shape) for k in names]

    def unflat(vec):
        out, o = {}, 0
        for k, s in zip(names, shapes):
            n = int(np.prod(s))
            out[k], o = vec[o:o + n].reshape(s), o + n
        return out

    init = {k: z[f"{tag}_init_{k}"] for k in names}
    online = [init] + [unflat(z[tag + "_params"][u]) for u in range(cfg["updates"])]
    gap = np.inf
    for u in range(cfg["updates"]):
        if v["is_double"] or v["freq"] == 0:
            sd = online[u]
        else:  # the target of process_fn u: synced at the start of learn u' for u' % freq == 0
            sd = init if u == 0 else unflat(z[tag + "_params_old"][u - 1])
        q = f64_forward(sd, store["obs_next"][idx[u]], v["K"])
        gap = min(gap, top2_gap(q.reshape(-1, v["A"])))
    assert gap >= cfg["min_gap"]
    assert gap == pytest.approx(chk["gap"], rel=1e-2)


def test_one_row_batch_keeps_its_batch_axis(z, cfg):
    """The deliberate difference: b == 1 with K > 1 means over branches and returns [1, K, A]
    (the reference's squeeze() gives [K, K, A])."""
    from tianshou_amd.data import Batch
    policy, v = make_policy(z, cfg, "double_target")
    vb, store = host_buffer(z, cfg, "double_target")
    idx = z["double_target_indices"][0][:5]
    many = policy._target_return(torch.as_tensor(store["obs_next"][idx]), store["rew"][idx],
                                 end_flags(vb, store, idx))
    one = policy._target_return(torch.as_tensor(store["obs_next"][idx[:1]]),
                                store["rew"][idx[:1]], end_flags(vb, store, idx[:1]))
    assert one.shape == (1,)  # a one-row GEMM may round differently from a five-row one
    np.testing.assert_allclose(one.numpy(), many[:1].numpy(), rtol=1e-5, atol=1e-6)

    class Buf:
        _save_obs_next = True
        _meta = Batch(rew=torch.as_tensor(store["rew"]),
                      done=torch.as_tensor(store["terminated"] | store["truncated"]))

        def _index_tensor(self, i):
            return torch.as_tensor(np.asarray(i, np.int64))

        def get(self, i, key):
            return torch.as_tensor(store[key][i])

        def _unfinished_device(self):
            return torch.as_tensor(vb.unfinished_index())

    batch = policy.process_fn(Batch(), Buf(), idx[:1])
    assert batch.returns.shape == (1, v["K"], v["A"])
    assert batch.returns.stride() == (1, 0, 0)  # a zero-copy expand
    assert torch.equal(batch.returns[0, 0, 0], one[0])


# -- network -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ("double_target", "one_branch"))
def test_seeded_construction_and_strict_load(z, cfg, tag):
    v = cfg["variants"][tag]
    torch.manual_seed(cfg["init_seed"])
    net = make_net(cfg, v)
    want = init_state(z, tag + "_init_")
    assert list(net.state_dict()) == list(want)
    for k, t in net.state_dict().items():
        assert torch.equal(t, want[k]), k
    assert [n for n, _ in net.named_children()] == ["common", "value", "branches"]
    assert isinstance(net.branches, torch.nn.ModuleList) and len(net.branches) == v["K"]
    other = make_net(cfg, v)
    other.load_state_dict(want, strict=True)
    assert len(list(net.parameters())) == 2 * (2 + 2 + v["K"] * 2)


def test_forward_follows_the_f64_restatement(z, cfg):
    v = cfg["variants"]["double_target"]
    net = make_net(cfg, v)
    net.load_state_dict(init_state(z, "double_target_init_"))
    obs = z["add_obs"][:37]
    logits, state = net(obs, state="s")
    assert state == "s" and logits.shape == (37, v["K"], v["A"]) and logits.dtype == torch.float32
    want = f64_forward({k: z["double_target_init_" + k] for k in net.state_dict()}, obs, v["K"])
    np.testing.assert_allclose(logits.detach().numpy(), want, rtol=1e-5, atol=1e-6)
    assert net.greedy_act(logits) is None  # the CPU runs the torch lines
    # the dueling aggregation: every branch's mean over actions is the state value
    np.testing.assert_allclose(logits.detach().numpy().mean(2),
                               np.repeat(want.mean(2)[:, :1], v["K"], 1), atol=1e-6)


def test_norm_args_and_act_args_are_refused_by_name():
    from tianshou_amd.utils.net import BranchingNet
    for name in ("norm_args", "act_args"):
        with pytest.raises(NotImplementedError, match=name):
            BranchingNet(4, 2, 3, [8], [8], [8], **{name: (1,)})
    net = BranchingNet(4, 2, 3, [8], [8], [8], torch.nn.LayerNorm, None, torch.nn.Tanh, None,
                       "cpu")
    kinds = [type(m).__name__ for m in net.common.model]
    assert kinds == ["Linear", "LayerNorm", "Tanh"]
    assert net(np.zeros((2, 4), np.float32))[0].shape == (2, 2, 3)


# -- policy surface ----------------------------------------------------------------------------------
def test_constructor_arguments_and_attributes():
    from tianshou_amd import policy as pol
    from tianshou_amd.policy import DQNPolicy
    from tianshou_amd.utils.net import BranchingNet
    net = BranchingNet(4, 3, 7, [8], [8], [8])
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    p = BranchingDQNPolicy(net, opt)
    assert isinstance(p, DQNPolicy) and "BranchingDQNPolicy" in pol.__all__
    assert (p._gamma, p._n_step, p._target, p._rew_norm, p._is_double) == \
        (0.99, 1, False, False, True)
    assert p.max_action_num == 7 and p.num_branches == 3 and p.eps == 0.0
    assert p._clip_loss_grad is False and p.fused_sample is False and p.fused is True
    p = BranchingDQNPolicy(net, opt, 0.9, 1, 5, False, False, action_space="ignored")
    assert (p._gamma, p._freq, p._is_double, p.action_space) == (0.9, 5, False, None)
    assert not p.model_old.training
    with pytest.raises(AssertionError, match="N-step bigger than one is not supported by BDQ"):
        BranchingDQNPolicy(net, opt, estimation_step=2)
    with pytest.raises(AssertionError, match="discount factor"):
        BranchingDQNPolicy(net, opt, discount_factor=1.5)


def test_forward_gives_the_first_index_argmax_per_branch():
    from tianshou_amd.data import Batch

    class Table(torch.nn.Module):
        num_branches, action_per_branch = 2, 3

        def forward(self, obs, state=None, **kw):
            return torch.as_tensor([[[1.0, 3.0, 3.0], [2.0, 2.0, 1.0]]]), state

    p = BranchingDQNPolicy(Table(), None)
    out = p(Batch(obs=np.zeros((1, 1), np.float32), info=Batch()))
    assert out.act.dtype == torch.int64 and out.act.tolist() == [[1, 0]]
    assert out.logits.shape == (1, 2, 3)


def test_exploration_noise_on_numpy_act_is_the_recordings(z):
    from tianshou_amd.data import Batch
    from tianshou_amd.utils.net import BranchingNet
    cases = json.loads(str(z["noise_cfg"]))
    assert len(cases) == 24
    for i, c in enumerate(cases):
        p = f"noise{i}_"
        policy = BranchingDQNPolicy(BranchingNet(3, c["K"], c["A"], [4], [4], [4]), None)
        policy.set_eps(c["eps"])
        act = z[p + "act_in"].copy()
        np.random.seed(c["seed"])
        got = policy.exploration_noise(act, Batch(obs=np.zeros((c["bsz"], 3), np.float32)))
        assert got is act
        np.testing.assert_array_equal(got, z[p + "act_out"], err_msg=p)
        st = np.random.get_state()
        np.testing.assert_array_equal(st[1], z[p + "state_keys"], err_msg=p)
        assert st[2] == int(z[p + "state_pos"]), p
        if c["eps"] == 1.0 and c["bsz"] > 1:
            assert not np.array_equal(got, z[p + "act_in"])
    # eps == 0 draws nothing
    policy.set_eps(0.0)
    np.random.seed(3)
    before = np.random.get_state()[2]
    assert policy.exploration_noise(act, Batch(obs=None)) is act
    assert np.random.get_state()[2] == before
    # obs.mask: the reference's host line adds the mask to the drawn actions
    policy = BranchingDQNPolicy(BranchingNet(3, 2, 4, [4], [4], [4]), None)
    policy.set_eps(1.0)
    act = np.zeros((5, 2), np.int64)
    mask = np.ones((5, 2), np.int64)
    np.random.seed(4)
    np.random.rand(5)
    want = np.random.randint(0, 4, (5, 2)) + 1
    np.random.seed(4)
    got = policy.exploration_noise(act, Batch(obs=Batch(obs=np.zeros((5, 3)), mask=mask)))
    np.testing.assert_array_equal(got, want)


def test_learn_act_hook_keeps_dqns_expression():
    from tianshou_amd.data import Batch
    from tianshou_amd.policy import DQNPolicy
    p = DQNPolicy(torch.nn.Linear(2, 3), None)
    dev = torch.device("cpu")
    for act in (torch.tensor([2, 0, 1]), torch.tensor([[2], [0], [1]]), np.array([2, 0, 1]),
                np.array([[2], [0], [1]], np.int32)):
        got = p._learn_act(Batch(act=act), dev, 3)
        want = torch.as_tensor(act, device=dev).reshape(3).to(torch.int64).contiguous()
        assert got.dtype == torch.int64 and got.shape == (3,) and torch.equal(got, want)
    from tianshou_amd.utils.net import BranchingNet
    b = BranchingDQNPolicy(BranchingNet(3, 2, 4, [4], [4], [4]), None)
    got = b._learn_act(Batch(act=np.array([[1, 2], [3, 0], [0, 0]], np.int32)), dev, 3)
    assert got.dtype == torch.int64 and got.tolist() == [[1, 2], [3, 0], [0, 0]]


def test_td_reference_matches_autograd_through_the_reference_lines():
    """Anchors ``td_reference`` (what the GPU tests compare the loss kernel with) against
    torch.autograd on bdq.py:115-124 in f64."""
    rng = np.random.default_rng(0)
    b, K, A = 9, 3, 4
    q = torch.tensor(rng.standard_normal((b, K, A)), requires_grad=True)
    act = rng.integers(0, A, (b, K))
    ret, w = rng.standard_normal(b), rng.random(b)
    mask = torch.zeros_like(q).scatter_(-1, torch.as_tensor(act).unsqueeze(-1), 1)
    td = torch.as_tensor(ret)[:, None, None].expand(b, K, A) * mask - q * mask
    loss = (td.pow(2).sum(-1).mean(-1) * torch.as_tensor(w)).mean()
    loss.backward()
    want_loss, want_prio, want_grad = td_reference(q.detach().numpy(), act, ret, w)
    np.testing.assert_allclose(loss.item(), want_loss, rtol=1e-12)
    np.testing.assert_allclose(td.sum(-1).sum(-1).detach().numpy(), want_prio, rtol=1e-12)
    np.testing.assert_allclose(q.grad.numpy(), want_grad, rtol=1e-12, atol=1e-300)


# -- spaces and the wrapper --------------------------------------------------------------------------
def test_multi_discrete_space():
    from tianshou_amd.env.spaces import MultiDiscrete
    sp = MultiDiscrete([3, 5, 2], seed=1)
    assert sp.nvec.tolist() == [3, 5, 2] and sp.nvec.dtype == np.int64
    assert sp.shape == (3,) and sp.dtype == np.int64
    draws = np.stack([sp.sample() for _ in range(200)])
    assert draws.dtype == np.int64 and draws.shape == (200, 3)
    assert (draws >= 0).all() and (draws < sp.nvec).all()
    assert [len(np.unique(draws[:, i])) for i in range(3)] == [3, 5, 2]
    assert sp.seed(1) == [1]
    again = np.stack([sp.sample() for _ in range(200)])
    np.testing.assert_array_equal(draws, again)
    np.random.seed(0)
    pos = np.random.get_state()[2]
    sp.sample()
    assert np.random.get_state()[2] == pos  # its own generator


def test_act_spec_of_a_multi_discrete_space():
    from tianshou_amd.data.collector import Collector
    from tianshou_amd.env.spaces import Box, Discrete, MultiDiscrete

    class Holder:
        _act_spec = Collector._act_spec

    h = Holder()
    for space, want in ((MultiDiscrete([4, 4, 4]), ((3,), torch.int64)),
                        (Discrete(5), ((), torch.int64)),
                        (Box(-1.0, 1.0, (2,)), ((2,), torch.float32)),
                        ([Discrete(2)] * 3, ((), torch.int64))):
        h._action_space = space
        assert h._act_spec() == want


def test_wrapper_mesh_is_the_references(z):
    from tianshou_amd.env.spaces import Box
    from tianshou_amd.env.synthetic import DeviceVectorEnv
    from tianshou_amd.env.wrappers import ContinuousToDiscrete
    w = json.loads(str(z["wrap_cfg"]))
    low, high = np.array(w["low"], np.float32), np.array(w["high"], np.float32)

    class BoxVenv(DeviceVectorEnv):
        env_num, device = 3, torch.device("cpu")
        action_space = Box(low, high, (2,))

        def step(self, action, id=None):
            return action

    for i, c in enumerate(w["cases"]):
        env = ContinuousToDiscrete(BoxVenv(), c["action_per_dim"])
        assert env.action_space.nvec.tolist() == c["nvec"] and len(env) == 3
        p = f"wrap{i}_"
        for d in range(2):
            np.testing.assert_array_equal(np.asarray(env.mesh[d], np.float64), z[p + f"mesh{d}"])
        for act, out in ((z[p + "act1"], z[p + "out1"]), (z[p + "act2"], z[p + "out2"])):
            got = env.action(act)
            assert got.dtype == torch.float32 and got.shape == out.shape
            np.testing.assert_array_equal(got.numpy(), out.astype(np.float32))
        assert torch.equal(env.step(z[p + "act2"]), env.action(z[p + "act2"]))
        table = env.mesh_t.numpy()
        assert table.shape == (2, max(c["nvec"])) and table.dtype == np.float32
        assert np.isnan(table).sum() == sum(max(c["nvec"]) - n for n in c["nvec"])
    with pytest.raises(AssertionError):
        ContinuousToDiscrete(BoxVenv(), [3, 3, 3])
    notbox = BoxVenv()
    notbox.action_space = env.action_space
    with pytest.raises(AssertionError):
        ContinuousToDiscrete(notbox, 3)


def test_new_symbols_are_declared_and_bound():
    from tianshou_amd import _C
    with open(os.path.join(ROOT, "include", "tsrl.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert name in _C._SIGS and name in _C.EXPORTED
        assert f" {name}(" in header
    assert len(_C._SIGS["tsrl_bdq_target"][0]) == 11
    assert len(_C._SIGS["tsrl_bdq_td_fwd_bwd"][0]) == 12
