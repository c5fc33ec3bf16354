"""DQNPolicy on the device path (tianshou_amd/policy/dqn.py, csrc/dqn.hip) against torch fp32
on the same device inputs (kernels) and against the reference run recorded in
tests/golden/dqn.npz (tools/gen_goldens.py gen_dqn; tests/test_dqn_host.py pins that file).

Kernel shapes are the lane, wave, workgroup and multi-partial edges (b 1 .. 1000, A 1 .. 65),
not workload sizes.  Tolerances: tsrl_dqn_target_q, td_error and tsrl_eps_greedy exact; loss
rtol 1e-5 / atol 1e-6, grad_q rtol 1e-4 / atol 1e-6 * max|grad| (DESIGN.md section 4's
loss-kernel tolerances).  update() against the recording: sampled indices equal, returns
rtol 1e-5 / atol 1e-6 (Q forwards on GPU GEMMs against CPU ones), losses rtol 2e-5 / atol
1e-6, Adam parameters rtol 1e-5 / atol 1e-6, prioritized weights rtol 1e-6 and tree leaves /
priorities rtol 1e-4 (|td|^alpha of f32 TD errors).  With RMSprop the parameter bound is 4 x
what the torch formulation of the same policy (``fused = False``: torch autograd +
torch.optim.RMSprop) deviates from the same recording on the same GPU (TORCH_DEV below)."""
import json
import os

import numpy as np
import pytest
import torch

from tianshou_amd import _C
from tianshou_amd.policy import DQNPolicy
from tianshou_amd.policy import dqn as dqn_mod
from tianshou_amd.policy.dqn import _DQNLoss, target_q_device

pytestmark = pytest.mark.gpu

# the entry points this file exercises (absent before DQNPolicy)
for _name in ("tsrl_dqn_target_q", "tsrl_dqn_td_fwd_bwd", "tsrl_dqn_num_partials",
              "tsrl_eps_greedy"):
    assert _name in _C.EXPORTED

# max |parameter - recorded| of the torch formulation (fused = False) after each of the six
# updates of the "rms" variant, measured on an MI355X against tests/golden/dqn.npz.  An early
# RMSprop step is lr * g / (0.1 |g| + eps): where |g| ~ eps it moves with the last bits of g.
TORCH_DEV = {
    "rms": (1.49e-8, 1.49e-8, 1.49e-8, 1.49e-8, 1.49e-8, 1.49e-8),
}
# (half an ulp of the largest parameters.)  The fused path measured 2.98e-8, 2.98e-8, 2.98e-8,
# 2.98e-8, 4.47e-8, 4.47e-8 in the same session, eager and graph-replayed alike.  The Adam
# variants, torch formulation: at most 1.49e-8 after every update of all four; fused: at most
# 2.98e-8 (double, notarget), 4.47e-8 (per) and 5.96e-8 (nature_huber) -- inside DESIGN.md
# section 4's rtol 1e-5 / atol 1e-6, so the 4 x rule is not needed there.

BS = (1, 63, 64, 65, 257, 1000)
AS = (1, 2, 6, 18, 65)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "dqn.npz"))


# -- kernels ------------------------------------------------------------------------------------
def _first_argmax(q: torch.Tensor) -> torch.Tensor:
    """The first index of each row's maximum (NumPy's documented argmax)."""
    return torch.as_tensor(q.cpu().numpy().argmax(axis=1), device=q.device)


@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("b", BS)
def test_target_q_matches_torch(dev, b, A):
    g = torch.Generator().manual_seed(1000 * b + A)
    rows = torch.arange(b, device=dev)
    cases = {
        "random": (torch.randn(b, A, generator=g), torch.randn(b, A, generator=g)),
        # few distinct values: most rows hold their maximum more than once
        "ties": (torch.randint(-2, 2, (b, A), generator=g).float() / 2,
                 torch.randn(b, A, generator=g)),
        "constant": (torch.full((b, A), 0.25), torch.randn(b, A, generator=g)),
        "negative": (-torch.rand(b, A, generator=g) - 0.5, -torch.rand(b, A, generator=g) - 0.5),
    }
    for name, (q_sel, q_eval) in cases.items():
        q_sel, q_eval = q_sel.to(dev), q_eval.to(dev)
        got = target_q_device(q_sel, q_eval, True)
        assert torch.equal(got, q_eval[rows, _first_argmax(q_sel)]), name
        if name == "random":  # no ties: torch's own formulation on the device
            assert torch.equal(got, q_eval.gather(1, q_sel.argmax(1, keepdim=True))[:, 0])
        assert torch.equal(target_q_device(None, q_eval, False), q_eval.max(dim=1)[0]), name
        # no target network: both arguments are the same tensor
        same = target_q_device(q_sel, q_sel, True)
        assert torch.equal(same, q_sel.max(dim=1)[0]), name
        assert torch.equal(target_q_device(q_sel, q_sel, False), same), name


def _td_inputs(b, A, kind, dev):
    g = torch.Generator().manual_seed(77 * b + A + len(kind))
    act = torch.randint(0, A, (b,), generator=g)
    weight = None
    if kind == "huber":
        # eighths: returns - q is exact, so |td| lands below, above and exactly on delta 1
        q = torch.randint(-16, 16, (b, A), generator=g).float() / 8
        td = torch.tensor([0.375, -0.5, 1.0, -1.0, 2.25, -3.0, 0.0])[torch.arange(b) % 7]
        returns = q[torch.arange(b), act] + td
    else:
        q = torch.randn(b, A, generator=g)
        returns = torch.randn(b, generator=g) * 2
        if kind == "mse_w":
            weight = torch.rand(b, generator=g) + 0.1
    d = lambda t: None if t is None else t.to(dev).contiguous()  # noqa: E731
    return d(q), d(act), d(returns), d(weight)


def _torch_td_loss(q, act, returns, weight, huber):
    """dqn.py:172-182 on the device."""
    qa = q[torch.arange(len(q), device=q.device), act]
    td = returns - qa
    if huber:
        loss = torch.nn.functional.huber_loss(qa.reshape(-1, 1), returns.reshape(-1, 1),
                                              reduction="mean")
    else:
        loss = (td.pow(2) * (1.0 if weight is None else weight)).mean()
    return loss, td


@pytest.mark.parametrize("kind", ("mse", "mse_w", "huber"))
@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("b", BS)
def test_td_fwd_bwd_matches_torch(dev, b, A, kind):
    q, act, returns, weight = _td_inputs(b, A, kind, dev)
    huber = kind == "huber"
    q_ref = q.clone().requires_grad_(True)
    loss_ref, td_ref = _torch_td_loss(q_ref, act, returns, weight, huber)
    loss_ref.backward()
    outs = []
    for _ in range(2):
        q_k = q.clone().requires_grad_(True)
        loss, td = _DQNLoss.apply(q_k, (act, returns, weight, huber, None, None))
        loss.backward()
        outs.append((loss.detach().clone(), td.clone(), q_k.grad.clone()))
    (loss, td, grad), again = outs
    if huber:
        assert (td.abs() == 1.0).any() == (b >= 3)
        assert b < 7 or ((td.abs() < 1.0).any() and (td.abs() > 1.0).any())
    print(f"b {b} A {A} {kind}: loss {loss.item():.7g} ref {loss_ref.item():.7g} "
          f"max|dgrad| {(grad - q_ref.grad).abs().max().item():.3g}")
    torch.testing.assert_close(loss, loss_ref.detach(), rtol=1e-5, atol=1e-6)
    assert torch.equal(td, td_ref.detach())
    gmax = float(q_ref.grad.abs().max())
    torch.testing.assert_close(grad, q_ref.grad, rtol=1e-4, atol=1e-6 * gmax)
    off = torch.ones_like(grad, dtype=torch.bool)
    off[torch.arange(b, device=dev), act] = False
    assert (grad[off] == 0).all()
    for a, c in zip(outs[0], again):  # a fixed summation order: the same bits every launch
        assert torch.equal(a, c)


def test_dqn_loss_seed_paths(dev):
    """_DQNLoss's backward under the learn path's constant unit seed hands the kernel's
    gradient over as it is; any other seed scales it (2.5 * loss)."""
    from tianshou_amd.policy.onpolicy import _unit_seed
    q, act, returns, weight = _td_inputs(257, 6, "mse_w", dev)
    grads = []
    for seed in ("ones", "unit", 2.5):
        q_k = q.clone().requires_grad_(True)
        loss, _ = _DQNLoss.apply(q_k, (act, returns, weight, False, None, None))
        if seed == "ones":
            loss.backward()
        elif seed == "unit":
            loss.backward(_unit_seed(dev))
        else:
            (loss * seed).backward()
        grads.append(q_k.grad.clone())
    assert torch.equal(grads[0], grads[1])
    torch.testing.assert_close(grads[2], 2.5 * grads[0], rtol=1e-6, atol=0)


def _noise_policy(A, eps, dev):
    policy = DQNPolicy(torch.nn.Linear(1, 1).to(dev), None)
    policy.max_action_num = A
    policy.set_eps(eps)
    return policy


def test_eps_greedy_matches_recorded_noise(z, dev):
    from tianshou_amd.data import Batch
    cases = json.loads(str(z["noise_cfg"]))
    assert len(cases) == 12
    for i, c in enumerate(cases):
        p = f"noise{i}_"
        policy = _noise_policy(c["A"], c["eps"], dev)
        act = torch.as_tensor(z[p + "act_in"], device=dev)
        obs = torch.zeros(c["bsz"], 1, device=dev)
        batch = Batch(obs=Batch(obs=obs, mask=z[p + "mask"]) if c["masked"] else obs)
        np.random.seed(c["seed"])
        out = policy.exploration_noise(act, batch)
        assert out.is_cuda and out.dtype == torch.int64
        np.testing.assert_array_equal(out.cpu().numpy(), z[p + "act_out"], err_msg=p)
        st = np.random.get_state()
        np.testing.assert_array_equal(st[1], z[p + "state_keys"], err_msg=p)
        assert st[2] == int(z[p + "state_pos"]), p
        # the host path (a NumPy act) from the same seed
        np.random.seed(c["seed"])
        host = policy.exploration_noise(z[p + "act_in"].copy(), Batch(
            obs=Batch(obs=obs, mask=z[p + "mask"]) if c["masked"] else obs))
        np.testing.assert_array_equal(host, z[p + "act_out"], err_msg=p)


def test_eps_greedy_eps_edges(dev):
    from tianshou_amd.data import Batch
    n, A = 257, 6
    act_in = torch.full((n,), A + 3, dtype=torch.int64, device=dev)  # no valid action
    batch = Batch(obs=torch.zeros(n, 1, device=dev))
    np.random.seed(5)
    before = np.random.get_state()
    out = _noise_policy(A, 0.0, dev).exploration_noise(act_in.clone(), batch)
    assert torch.equal(out, act_in)  # eps 0: untouched,
    after = np.random.get_state()
    assert np.array_equal(before[1], after[1]) and before[2] == after[2]  # and nothing drawn
    out = _noise_policy(A, 1.0, dev).exploration_noise(act_in.clone(), batch)
    assert bool(((out >= 0) & (out < A)).all())  # eps 1: every row replaced


# -- update() against the recording -----------------------------------------------------------------
def _cfg(z):
    return json.loads(str(z["learn_cfg"]))


def _filled_buffer(z, cfg, dev, per=False):
    from tianshou_amd.data import Batch, PrioritizedVectorReplayBuffer, VectorReplayBuffer
    E, S = cfg["E"], cfg["S"]
    buf = PrioritizedVectorReplayBuffer(E * S, E, alpha=0.6, beta=0.4, device=dev) if per \
        else VectorReplayBuffer(E * S, E, device=dev)
    o = 0
    for k in z["add_len"]:
        sl = slice(o, o + int(k))
        buf.add(Batch(**{key: z["add_" + key][sl] for key in
                         ("obs", "act", "rew", "terminated", "truncated", "obs_next")}),
                buffer_ids=z["add_ids"][sl])
        o += int(k)
    assert buf._lengths.tolist() == z["buf_lengths"].tolist()
    assert buf.last_index.tolist() == z["buf_last_index"].tolist()
    return buf


def _policy(z, cfg, tag, dev, optim=None, **attrs):
    from tianshou_amd.utils.net import Net
    v = cfg["variants"][tag]
    net = Net(cfg["D"], cfg["A"], hidden_sizes=tuple(cfg["hidden"]), device=dev).to(dev)
    net.load_state_dict({k[len("init_"):]: torch.as_tensor(z[k]) for k in z.files
                         if k.startswith("init_")})
    if optim is None:
        optim = "rms" if v["optim"] == "rms" else "adam"
    opt = {"rms": lambda p: torch.optim.RMSprop(p, lr=7e-4, eps=1e-5, alpha=0.99),
           "adam": lambda p: torch.optim.Adam(p, lr=1e-3),
           "sgd": lambda p: torch.optim.SGD(p, lr=1e-2)}[optim](net.parameters())
    policy = DQNPolicy(net, opt, discount_factor=cfg["gamma"], estimation_step=v["n_step"],
                       target_update_freq=v["freq"], is_double=v["is_double"],
                       clip_loss_grad=v["huber"]).to(dev)
    for k, a in attrs.items():
        setattr(policy, k, a)
    return policy, v


def _record(policy):
    """Wrap process_fn / learn so each update leaves its indices, returns, weight and TD
    errors in the returned list."""
    process_fn, learn, seen = policy.process_fn, policy.learn, []

    def rec_process(batch, buffer, indices):
        batch = process_fn(batch, buffer, indices)
        seen.append(dict(indices=np.array(indices, copy=True), returns=batch.returns.clone()))
        if "weight" in batch:
            seen[-1]["weight"] = batch.weight.clone()
        return batch

    def rec_learn(batch, **kw):
        res = learn(batch, **kw)
        seen[-1]["td_error"] = batch.weight.clone()
        return res

    policy.process_fn, policy.learn = rec_process, rec_learn
    return seen


def _param_dev(module, z, prefix):
    worst = 0.0
    for k, t in module.state_dict().items():
        e = np.abs(t.detach().cpu().numpy().astype(np.float64) - z[prefix + k]).max()
        worst = max(worst, float(e))
    return worst


def _run_variant(z, dev, tag, check_params, **attrs):
    """Six update() calls of one recorded variant; everything but the parameters is asserted
    here, the parameters by ``check_params(u, policy)``."""
    cfg = _cfg(z)
    policy, v = _policy(z, cfg, tag, dev, **attrs)
    buf = _filled_buffer(z, cfg, dev, per=bool(v.get("per")))
    seen = _record(policy)
    np.random.seed(cfg["seed"])
    losses = []
    for u in range(6):
        res = policy.update(v["bs"], buf)
        q = f"{tag}_u{u}_"
        s = seen[u]
        assert s["indices"].tolist() == z[q + "indices"].tolist(), q
        print(f"{q} loss {res['loss']:.7g} recorded {float(z[q + 'loss']):.7g} "
              f"max|dparam| {_param_dev(policy.model, z, q + 'param_'):.3g}")
        np.testing.assert_allclose(s["returns"].cpu().numpy(), z[q + "returns"], rtol=1e-5,
                                   atol=1e-6, err_msg=q)
        np.testing.assert_allclose(res["loss"], float(z[q + "loss"]), rtol=2e-5, atol=1e-6,
                                   err_msg=q)
        assert s["td_error"].is_cuda and not s["td_error"].requires_grad
        # td = returns - Q(s, a): a difference of two quantities each inside the returns bound
        td_atol = 2 * (1e-5 * float(np.abs(z[q + "returns"]).max()) + 1e-6)
        np.testing.assert_allclose(s["td_error"].cpu().numpy(), z[q + "td_error"], rtol=0,
                                   atol=td_atol, err_msg=q)
        if v.get("per"):
            np.testing.assert_allclose(s["weight"].cpu().numpy(), z[q + "weight"], rtol=1e-6,
                                       err_msg=q)
            leaves = buf.weight[np.arange(buf.maxsize)]
            np.testing.assert_allclose(np.asarray(leaves), z[q + "leaves"], rtol=1e-4,
                                       err_msg=q)
        check_params(u, policy)
        losses.append(res["loss"])
    if v.get("per"):
        np.testing.assert_allclose(buf._max_prio, float(z[tag + "_max_prio"]), rtol=1e-4)
        np.testing.assert_allclose(buf._min_prio, float(z[tag + "_min_prio"]), rtol=1e-4)
    assert policy._iter == 6
    return policy, losses


def _adam_check(z, tag):
    def check(u, policy):
        for k, t in policy.model.state_dict().items():
            np.testing.assert_allclose(t.cpu().numpy(), z[f"{tag}_u{u}_param_{k}"], rtol=1e-5,
                                       atol=1e-6, err_msg=f"{tag} update {u} {k}")
        if tag == "double" and u == 4:
            # the sync at _iter 3: model_old holds the online parameters from before update
            # 3's step (recorded after update 2), untouched by update 4
            for k, t in policy.model_old.state_dict().items():
                np.testing.assert_allclose(t.cpu().numpy(), z[f"{tag}_u2_param_{k}"],
                                           rtol=1e-5, atol=1e-6, err_msg=f"model_old {k}")
            assert not any(torch.equal(a, b) for a, b in zip(policy.model.parameters(),
                                                             policy.model_old.parameters()))
    return check


@pytest.mark.parametrize("tag", ("double", "nature_huber", "notarget", "per"))
def test_update_matches_reference_adam(z, dev, tag):
    policy, _ = _run_variant(z, dev, tag, _adam_check(z, tag))
    assert policy._flat is not None and policy._flat.adam_bound(policy.optim)
    assert policy._learn_graphs and not policy._graph_failed  # 64-row updates replay


def test_update_matches_reference_rmsprop(z, dev):
    """Measured on an MI355X, max |parameter - recorded| after each update: see TORCH_DEV and
    the figures this test prints."""
    def check(u, policy):
        d = _param_dev(policy.model, z, f"rms_u{u}_param_")
        assert d <= 4 * TORCH_DEV["rms"][u], (u, d)
    policy, _ = _run_variant(z, dev, "rms", check)
    assert policy._flat.adam_bound(policy.optim)
    assert set(policy.optim.state[next(policy.model.parameters())]) == {"step", "square_avg"}


@pytest.mark.parametrize("tag", ("double", "nature_huber", "per"))
def test_torch_formulation_matches_reference(z, dev, tag):
    """fused = False, the reference's op sequence on the GPU (the benchmark's comparison
    leg), meets the same bounds."""
    policy, _ = _run_variant(z, dev, tag, _adam_check(z, tag), fused=False)
    assert policy._flat is None and not policy._learn_graphs


# -- paths taken ------------------------------------------------------------------------------------
def test_flat_storage_is_bound_with_plain_adam(z, dev):
    cfg = _cfg(z)
    policy, v = _policy(z, cfg, "double", dev)
    buf = _filled_buffer(z, cfg, dev)
    np.random.seed(3)
    policy.update(v["bs"], buf)
    fa = policy._flat
    assert fa is not None and fa.adam_bound(policy.optim)
    flat = fa.flat_param
    lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * 4
    for p in policy.model.parameters():
        assert lo <= p.data_ptr() < hi
        st = policy.optim.state[p]
        for name in ("exp_avg", "exp_avg_sq"):
            assert st[name].shape == p.shape and st[name]._base is not None
    old = policy._old_flat
    assert old is not None and old.shape == flat.shape
    storages = {p.untyped_storage().data_ptr() for p in policy.model_old.parameters()}
    assert storages == {old.untyped_storage().data_ptr()}
    policy.update(v["bs"], buf)
    assert not torch.equal(old, flat)
    policy.sync_weight()
    assert torch.equal(old, flat)
    for a, b in zip(policy.model.parameters(), policy.model_old.parameters()):
        assert torch.equal(a, b)
    assert not policy.model_old.training and policy.train().model.training
    assert not policy.model_old.training


def test_other_optimisers_keep_torch_step(z, dev):
    cfg = _cfg(z)
    policy, v = _policy(z, cfg, "double", dev, optim="sgd")
    buf = _filled_buffer(z, cfg, dev)
    before = [p.detach().clone() for p in policy.model.parameters()]
    np.random.seed(3)
    losses = [policy.update(v["bs"], buf)["loss"] for _ in range(3)]
    assert policy._flat is None or not policy._flat.adam_bound(policy.optim)
    assert not policy._learn_graphs
    assert all(np.isfinite(losses)) and len(set(losses)) == 3
    assert all(not torch.equal(a, b) for a, b in zip(before, policy.model.parameters()))


def _six_updates(z, dev, tag, sizes, **attrs):
    cfg = _cfg(z)
    policy, v = _policy(z, cfg, tag, dev, **attrs)
    buf = _filled_buffer(z, cfg, dev, per=bool(v.get("per")))
    np.random.seed(cfg["seed"])
    losses = [policy.update(bs, buf)["loss"] for bs in sizes]
    return policy, losses, [p.detach().clone() for p in policy.model.parameters()]


@pytest.mark.parametrize("tag", ("double", "nature_huber", "per"))
def test_graph_replay_is_bitwise_eager(z, dev, tag):
    bs = _cfg(z)["variants"][tag]["bs"]
    pol_g, loss_g, par_g = _six_updates(z, dev, tag, [bs] * 6, graph_learn=True)
    pol_e, loss_e, par_e = _six_updates(z, dev, tag, [bs] * 6, graph_learn=False)
    assert len(pol_g._learn_graphs) == 1 and not pol_e._learn_graphs
    assert loss_g == loss_e
    for a, b in zip(par_g, par_e):
        assert torch.equal(a, b)


def test_graph_replay_follows_batch_size(z, dev):
    sizes = [64, 64, 32, 64, 48, 32]
    pol_g, loss_g, par_g = _six_updates(z, dev, "double", sizes, graph_learn=True)
    pol_e, loss_e, par_e = _six_updates(z, dev, "double", sizes, graph_learn=False)
    assert sorted(k[0] for k in pol_g._learn_graphs) == [32, 48, 64]
    assert loss_g == loss_e
    for a, b in zip(par_g, par_e):
        assert torch.equal(a, b)


def test_capture_failure_warns_once_and_stays_eager(z, dev, monkeypatch):
    """A capture that raises RuntimeError (simulated on the host: the capture entry raises
    before torch.cuda.graph is entered, so no stream is ever capturing) warns once, latches
    _graph_failed and every update runs eagerly, still matching the recording."""
    import warnings
    tries = []

    def failing_capture(graph):
        tries.append(graph)
        raise RuntimeError("simulated capture failure")

    monkeypatch.setattr(dqn_mod, "graph_capture", failing_capture)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        policy, _ = _run_variant(z, dev, "double", _adam_check(z, "double"), graph_learn=True)
    msgs = [w for w in caught if "learn-graph capture failed" in str(w.message)]
    assert len(msgs) == 1 and len(tries) == 1
    assert policy._graph_failed and not policy._learn_graphs


# -- Collector --------------------------------------------------------------------------------------
def _cartpole(z, dev, buf, noise, seed_offset=0):
    from tianshou_amd.data import Collector
    from tianshou_amd.env import CartPoleEnv, Discrete, DummyVectorEnv
    from tianshou_amd.utils.net import Net
    c = json.loads(str(z["col_cfg"]))
    envs = DummyVectorEnv([CartPoleEnv for _ in range(c["E"])])
    seed = c["seed"] + seed_offset
    np.random.seed(seed)
    torch.manual_seed(seed)
    envs.seed(seed)
    net = Net(4, 2, hidden_sizes=(16, 16), device=dev).to(dev)
    policy = DQNPolicy(net, torch.optim.Adam(net.parameters(), lr=1e-3), target_update_freq=10,
                       action_space=Discrete(2)).to(dev)
    return c, policy, Collector(policy, envs, buf, exploration_noise=noise)


def test_collect_eps_one_matches_reference(z, dev):
    """At eps 1.0 every action comes from NumPy's stream alone, so the trajectory does not
    depend on f32 Q-values: buffer and episode statistics bit for bit."""
    from tianshou_amd.data import VectorReplayBuffer
    c = json.loads(str(z["col_cfg"]))
    buf = VectorReplayBuffer(c["size"], c["E"], device=dev)
    _, policy, col = _cartpole(z, dev, buf, noise=True)
    policy.set_eps(1.0)
    res = col.collect(n_step=c["n_step"])
    assert res["n/ep"] == int(z["col_n_ep"]) and res["n/st"] == int(z["col_n_st"])
    for k in ("lens", "idxs", "rews"):
        assert np.asarray(res[k]).tolist() == z["col_" + k].tolist(), k
    m = buf._meta
    for k in ("obs", "obs_next", "act", "rew", "terminated", "truncated", "done"):
        got, want = getattr(m, k).cpu().numpy(), z["col_buf_" + k]
        assert got.shape == want.shape, k
        assert np.array_equal(got.astype(want.dtype), want), k


def test_collect_greedy_then_prioritized_updates(z, dev):
    from tianshou_amd.data import PrioritizedVectorReplayBuffer
    c = json.loads(str(z["col_cfg"]))
    E, n_step = c["E"], 120
    buf = PrioritizedVectorReplayBuffer(c["size"], E, alpha=0.6, beta=0.4, device=dev)
    _, policy, col = _cartpole(z, dev, buf, noise=False, seed_offset=1)
    policy.set_eps(1.0)  # ignored: this collector applies no exploration noise
    res = col.collect(n_step=n_step)
    assert res["n/st"] == n_step
    steps, S = n_step // E, buf.maxsize // E
    m = buf._meta
    with torch.no_grad():
        for t in range(steps):  # the collector's own batches: one row per env
            rows = torch.arange(E, device=dev) * S + t
            q, _ = policy.model(m.obs[rows])
            assert torch.equal(m.act[rows].reshape(-1), q.argmax(dim=1)), t
    np.random.seed(4)
    losses = [policy.update(64, buf)["loss"] for _ in range(3)]
    assert all(np.isfinite(losses)) and len(set(losses)) == 3
