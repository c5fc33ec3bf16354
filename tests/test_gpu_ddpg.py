"""DDPGPolicy / TD3Policy on the device path (tianshou_amd/policy/ddpg.py, td3.py,
csrc/ddpg.hip) against torch fp32 on the same device inputs and f64 restatements (kernels), and
against the reference run recorded in tests/golden/ddpg.npz (tools/gen_goldens.py gen_ddpg;
tests/test_ddpg_host.py pins that file).

Kernel shapes are the lane, wave, workgroup, float4-body and multi-partial edges, not workload
sizes.  Tolerances: tsrl_soft_update, tsrl_td3_smooth, tsrl_act_noise and the per-row vector
of tsrl_q_mse_fwd_bwd bitwise; losses rtol 1e-5, gradients rtol 1e-4 / atol 1e-6 * max|ref|
(DESIGN.md section 4's loss-kernel tolerances); -mean(q) within 1e-5 * mean|q|.  update()
against the recording: sampled indices, _cnt and the actor-step schedule equal, returns rtol
1e-5, critic losses rtol 2e-5, actor loss within 2e-5 * mean|Q| of the recorded critic outputs
(a signed mean), outgoing weights rtol 1e-4, Adam parameters (online and target) rtol 1e-5 /
atol 1e-6, prioritized weights rtol 1e-6 and tree leaves / priorities rtol 1e-4.  With RMSprop
the parameter bound is 4 x what the torch formulation of the same policy (``fused = False``)
deviates from the same recording on the same GPU (TORCH_DEV below)."""
import json
import warnings

import numpy as np
import pytest
import torch

from tests import ddpg_common as common
from tianshou_amd import _C
from tianshou_amd.policy import DDPGPolicy
from tianshou_amd.policy import ddpg as ddpg_mod
from tianshou_amd.policy.ddpg import (act_noise_device, neg_mean_loss, q_mse_loss,
                                      soft_update_device)
from tianshou_amd.policy.td3 import td3_smooth_device

pytestmark = pytest.mark.gpu

for _name in ("tsrl_soft_update", "tsrl_td3_smooth", "tsrl_q_mse_fwd_bwd",
              "tsrl_neg_mean_fwd_bwd", "tsrl_act_noise", "tsrl_ddpg_num_partials"):
    assert _name in _C.EXPORTED

# max |parameter - recorded| (online and target networks) of the torch formulation
# (fused = False) after each of the six updates of the "ddpg_rms" variant, measured on an
# MI355X against tests/golden/ddpg.npz.  An early RMSprop step is lr * g / (0.1 |g| + eps):
# where |g| ~ eps it moves with the last bits of g.
TORCH_DEV = {
    "ddpg_rms": (1.49e-8, 2.98e-8, 2.98e-8, 2.98e-8, 2.98e-8, 2.98e-8),
}
# (half an ulp and one ulp of the largest parameters.)  The fused path measured 2.98e-8 after
# every update in the same session.  The Adam variants, fused: at most 5.96e-8 -- inside rtol
# 1e-5 / atol 1e-6, so the 4 x rule is not needed there.

BS = (1, 63, 64, 65, 257, 1000)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def z(golden_dir):
    return common.golden(golden_dir)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


# -- tsrl_soft_update -------------------------------------------------------------------------------
def _segments(n, nseg, shift):
    """(length, target offset, source offset) of nseg segments at odd element offsets into
    shared flat buffers; ``shift`` moves the sources so that target and source are misaligned
    differently (the kernel's all-scalar path)."""
    lens = [n, (3 * n) // 4 + 1, 5, n // 3 + 2][:nseg]
    segs, o = [], 1
    for k in lens:
        segs.append((k, o, o + shift))
        o += k + 2 + (k % 2)  # the next offset is odd again
    return segs, o + 8


@pytest.mark.parametrize("tau", (0.0, 0.005, 0.5, 1.0))
@pytest.mark.parametrize("n", (1, 255, 256, 257, 4097, 70001))
def test_soft_update_matches_torch_bitwise(dev, n, tau):
    g = torch.Generator().manual_seed(n)
    for nseg in (1, 3, 4):
        for shift in (0, 1, 2):
            segs, total = _segments(n, nseg, shift)
            assert all(o % 2 == 1 for _, o, _ in segs)
            tgt = torch.randn(total, generator=g).to(dev)
            src = torch.randn(total, generator=g).to(dev)
            want = tgt.clone()
            for k, ot, os_ in segs:
                s, t = src[os_:os_ + k], tgt[ot:ot + k]
                want[ot:ot + k] = tau * s + (1 - tau) * t  # BasePolicy.soft_update's expression
            src_before = src.clone()
            soft_update_device([(tgt[ot:ot + k], src[os_:os_ + k]) for k, ot, os_ in segs], tau)
            assert torch.equal(_bits(tgt), _bits(want)), (nseg, shift)  # gaps untouched too
            assert torch.equal(src, src_before)
    if tau == 1.0:
        assert torch.equal(tgt[segs[0][1]:segs[0][1] + n], src[segs[0][2]:segs[0][2] + n])


def test_soft_update_rejects_bad_arguments(dev):
    t, s = torch.zeros(8, device=dev), torch.zeros(8, device=dev)
    with pytest.raises(_C.TsrlError, match="tau"):
        soft_update_device([(t, s)], 1.5)
    with pytest.raises(ValueError):
        soft_update_device([(t, s[:4])], 0.5)
    soft_update_device([], 0.5)
    # five pairs: two launches
    ts = [torch.full((3,), float(i), device=dev) for i in range(5)]
    ss = [torch.full((3,), 10.0, device=dev) for _ in range(5)]
    soft_update_device(list(zip(ts, ss)), 0.5)
    for i, x in enumerate(ts):
        assert torch.equal(x, torch.full((3,), 0.5 * 10.0 + 0.5 * i, device=dev))


def _perturbed_td3(z, dev, **attrs):
    cfg = common.learn_cfg(z)
    policy, v = common.make_policy(z, cfg, "td3", dev, **attrs)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for name in policy._sync_order:  # online and target networks apart
            for p in getattr(policy, name).parameters():
                p.add_(0.1 * torch.randn(p.shape, generator=g).to(dev))
    return policy, cfg, v


def test_sync_weight_matches_base_soft_update(z, dev):
    from copy import deepcopy
    from tianshou_amd.policy import BasePolicy
    policy, cfg, _ = _perturbed_td3(z, dev)
    for name in policy._sync_order:
        assert policy._bind(name) is not None
    ref = {name: deepcopy(getattr(policy, name + "_old")) for name in policy._sync_order}
    for _ in range(2):
        policy.sync_weight()
        for name in policy._sync_order:
            BasePolicy.soft_update(policy, ref[name], getattr(policy, name), policy.tau)
    for name in policy._sync_order:
        assert policy._flat_pair(name) is not None
        for a, b in zip(getattr(policy, name + "_old").parameters(), ref[name].parameters()):
            assert torch.equal(_bits(a.detach()), _bits(b.detach())), name
        assert not any(torch.equal(a, b) for a, b in zip(
            getattr(policy, name).parameters(), getattr(policy, name + "_old").parameters()))


# -- tsrl_td3_smooth --------------------------------------------------------------------------------
@pytest.mark.parametrize("A", (1, 3, 6, 17))
@pytest.mark.parametrize("b", (1, 63, 64, 65, 257))
def test_td3_smooth_matches_torch_bitwise(dev, b, A):
    g = torch.Generator().manual_seed(100 * b + A)
    act = (torch.rand(b, A, generator=g) * 2 - 1).to(dev)
    noise = torch.randn(b, A, generator=g).to(dev)
    if b * A >= 3:  # both sides of the clip and a NaN, whatever the draw
        flat = noise.view(-1)
        flat[0], flat[1], flat[2] = 9.0, -9.0, float("nan")
    for sigma, clip in ((0.2, 0.0), (0.2, 0.1), (0.7, 0.5), (0.0, 0.5), (0.0, 0.0)):
        want = noise * sigma  # td3.py:101-104
        if clip > 0.0:
            want = want.clamp(-clip, clip)
        want = act + want
        if clip > 0.0 and sigma > 0.0 and b * A >= 3:
            d = (want - act).view(-1)
            assert d[0] > 0 and d[1] < 0 and abs(float(d[0]) - clip) < 1e-6
        got = td3_smooth_device(act.clone(), noise, sigma, clip)
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan), (sigma, clip)
        assert bool(nan.any()) == (b * A >= 3)
        assert torch.equal(_bits(got)[~nan], _bits(want)[~nan]), (sigma, clip)


# -- tsrl_act_noise and exploration_noise -----------------------------------------------------------------
def test_act_noise_matches_recorded_noise(z, dev):
    """The kernel over the host's own draws (tests/test_ddpg_host.py holds those to the
    reference bit for bit) and exploration_noise on a device and a NumPy ``act``, every case
    of the recording: the reference's f64 result rounded to f32, NumPy's state as it left it."""
    from tianshou_amd.data import Batch
    for i, c in enumerate(common.noise_cases(z)):
        p = f"noise{i}_"
        act = z[p + "act_in"]
        act_d = torch.as_tensor(act, device=dev)
        policy = DDPGPolicy(None, None, None, None, exploration_noise=common.make_noise(c),
                            action_scaling=False)
        np.random.seed(c["seed"])
        for call in range(c["calls"]):
            out = policy.exploration_noise(act_d, Batch())
            if c["kind"] == "none":
                assert out is act_d
                continue
            want = z[p + "act_out"][call]
            assert out.is_cuda and out.dtype == torch.float32 and out.shape == act_d.shape
            np.testing.assert_array_equal(out.cpu().numpy(), want.astype(np.float32),
                                          err_msg=f"{p}{call}")
            noise = want - act.astype(np.float64)  # not the draw itself, but a valid f64 input
            direct = act_noise_device(act_d, noise)
            np.testing.assert_array_equal(
                direct.cpu().numpy(), (act.astype(np.float64) + noise).astype(np.float32))
        common.assert_np_state(z, p)
        assert torch.equal(act_d, torch.as_tensor(act, device=dev))  # the input is not written
        host = DDPGPolicy(None, None, None, None, exploration_noise=common.make_noise(c),
                          action_scaling=False)
        np.random.seed(c["seed"])
        for call in range(c["calls"]):
            out = host.exploration_noise(act, Batch())
            if c["kind"] == "none":
                assert out is act
            else:
                np.testing.assert_array_equal(out, z[p + "act_out"][call])
        common.assert_np_state(z, p)


# -- tsrl_q_mse_fwd_bwd -----------------------------------------------------------------------------
def _q_inputs(b, nc, weighted, dev, constructed=False):
    g = torch.Generator().manual_seed(31 * b + 7 * nc + weighted)
    qs = [torch.randn(b, generator=g) for _ in range(nc)]
    returns = torch.randn(b, generator=g) * 2
    weight = torch.rand(b, generator=g) + 0.1 if weighted else None
    if constructed:  # td = 0, a huge td, a zero weight
        qs[0][0] = returns[0]
        qs[-1][1] = returns[1] + 3e18
        if weight is not None:
            weight[2] = 0.0
    d = lambda t: None if t is None else t.to(dev).contiguous()  # noqa: E731
    return [d(q) for q in qs], d(returns), d(weight)


def _q_mse_f64(qs, returns, weight):
    """ddpg.py:173-178 in f64: (losses, gradients) per critic."""
    r = returns.double()
    w = torch.ones_like(r) if weight is None else weight.double()
    losses, grads = [], []
    for q in qs:
        td = q.double() - r
        losses.append((td * td * w).sum() / len(r))
        grads.append(2.0 * td * w / len(r))
    return losses, grads


def _check_q_mse(dev, b, nc, weighted, constructed):
    qs, returns, weight = _q_inputs(b, nc, weighted, dev, constructed)
    loss64, grad64 = _q_mse_f64(qs, returns, weight)
    # torch fp32 beside it
    q_ref = [q.clone().requires_grad_(True) for q in qs]
    tds = [q - returns for q in q_ref]
    loss_ref = [(td.pow(2) * (1.0 if weight is None else weight)).mean() for td in tds]
    sum(loss_ref).backward()
    row_ref = tds[0].detach() if nc == 1 else ((tds[0] + tds[1]) / 2.0).detach()
    outs = []
    for _ in range(2):
        q_k = [q.clone().requires_grad_(True) for q in qs]
        handle, loss, row = q_mse_loss(q_k, returns, weight)
        handle.backward()
        outs.append((loss.clone(), row.clone(), handle.detach().clone(),
                     *(q.grad.clone() for q in q_k)))
    loss, row, total = outs[0][:3]
    grads = outs[0][3:]
    for k in range(nc):
        gmax = float(grad64[k].abs().max())
        print(f"b {b} critics {nc} weighted {weighted} constructed {constructed} [{k}]: loss "
              f"{loss[k].item():.7g} f64 {loss64[k].item():.7g} torch {loss_ref[k].item():.7g} "
              f"max|dgrad| {(grads[k].double() - grad64[k]).abs().max().item():.3g} torch "
              f"{(q_ref[k].grad.double() - grad64[k]).abs().max().item():.3g} of {gmax:.3g}")
        torch.testing.assert_close(loss[k].double(), loss64[k], rtol=1e-5, atol=0)
        torch.testing.assert_close(grads[k].double(), grad64[k], rtol=1e-4, atol=1e-6 * gmax)
    torch.testing.assert_close(total.double(), sum(loss64), rtol=1e-5, atol=0)
    assert torch.equal(_bits(row), _bits(row_ref))
    for a, c in zip(outs[0], outs[1]):  # a fixed summation order: the same bits every launch
        assert torch.equal(_bits(a), _bits(c))
    return qs, returns, weight, loss, grads, row


@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("nc", (1, 2))
@pytest.mark.parametrize("b", BS)
def test_q_mse_matches_f64(dev, b, nc, weighted):
    _check_q_mse(dev, b, nc, weighted, constructed=False)


@pytest.mark.parametrize("nc", (1, 2))
@pytest.mark.parametrize("b", (65, 1000))
def test_q_mse_constructed_rows(dev, b, nc):
    qs, returns, weight, loss, grads, row = _check_q_mse(dev, b, nc, True, constructed=True)
    assert float(grads[0][0]) == 0.0 and (nc == 2 or float(row[0]) == 0.0)  # td = 0
    assert all(float(g[2]) == 0.0 for g in grads)  # zero weight: no gradient
    assert float(row[2]) != 0.0
    assert float(row[1].abs()) > 1e18 and torch.isfinite(loss).all()
    assert float(loss[-1]) > 1e30


def test_q_mse_seed_paths(dev):
    """backward under the learn path's constant unit seed hands the kernel's gradients over
    as they are; any other seed scales them."""
    from tianshou_amd.policy.onpolicy import _unit_seed
    qs, returns, weight = _q_inputs(257, 2, True, dev)
    grads = []
    for seed in ("ones", "unit", 2.5):
        q_k = [q.clone().requires_grad_(True) for q in qs]
        handle, _, _ = q_mse_loss(q_k, returns, weight)
        if seed == "ones":
            handle.backward()
        elif seed == "unit":
            handle.backward(_unit_seed(dev))
        else:
            (handle * seed).backward()
        grads.append([q.grad.clone() for q in q_k])
    for k in range(2):
        assert torch.equal(grads[0][k], grads[1][k])
        torch.testing.assert_close(grads[2][k], 2.5 * grads[0][k], rtol=1e-6, atol=0)


# -- tsrl_neg_mean_fwd_bwd ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("random", "cancelling"))
@pytest.mark.parametrize("b", BS)
def test_neg_mean_matches_f64(dev, b, kind):
    g = torch.Generator().manual_seed(b)
    q = torch.randn(b, generator=g) * 3 + 0.5
    if kind == "cancelling" and b > 1:  # pairs that cancel but for 1e-3
        h = b // 2
        q[:h] = torch.randn(h, generator=g) * 50
        q[h:2 * h] = -q[:h] + 1e-3
        q = q[torch.randperm(b, generator=g)]
    q = q.to(dev)
    want = -(q.double().sum() / b)
    outs = []
    for _ in range(2):
        q_k = q.clone().requires_grad_(True)
        loss = neg_mean_loss(q_k)
        loss.backward()
        outs.append((loss.detach().clone(), q_k.grad.clone()))
    loss, grad = outs[0]
    q_t = q.clone().requires_grad_(True)
    loss_t = -q_t.mean()
    loss_t.backward()
    scale = float(q.abs().double().mean())
    print(f"b {b} {kind}: loss {loss.item():.7g} f64 {want.item():.7g} torch {loss_t.item():.7g} "
          f"mean|q| {scale:.4g}")
    assert abs(float(loss) - float(want)) <= 1e-5 * scale
    exact = torch.full((b,), float(np.float32(-1.0) / np.float32(b)), device=dev)
    assert torch.equal(_bits(grad), _bits(exact))
    assert torch.equal(grad, torch.full((b,), -1.0 / b, dtype=torch.float32, device=dev))
    assert torch.equal(grad, q_t.grad)
    for a, c in zip(outs[0], outs[1]):
        assert torch.equal(_bits(a), _bits(c))
    # into a static output: the loss lands there
    slot = torch.zeros(3, device=dev)
    neg_mean_loss(q.clone().requires_grad_(True), slot[2:])
    assert torch.equal(slot[2], loss) and float(slot[:2].abs().sum()) == 0.0


# -- update() against the recording -----------------------------------------------------------------
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


def _record(policy):
    process_fn, learn, seen = policy.process_fn, policy.learn, []

    def rec_process(batch, buffer, indices):
        batch = process_fn(batch, buffer, indices)
        seen.append(dict(indices=np.array(indices, copy=True), returns=batch.returns.clone()))
        if "weight" in batch:
            seen[-1]["weight"] = batch.weight.clone()
        return batch

    def rec_learn(batch, **kw):
        res = learn(batch, **kw)
        seen[-1]["td"] = batch.weight.clone()
        return res

    policy.process_fn, policy.learn = rec_process, rec_learn
    return seen


def _setup(z, dev, tag, **attrs):
    cfg = common.learn_cfg(z)
    policy, v = common.make_policy(z, cfg, tag, dev, **attrs)
    if v["kind"] == "td3":
        common.feed_draws(policy, z[tag + "_randn"])
    return cfg, policy, v, _filled_buffer(z, cfg, dev, per=bool(v.get("per")))


def _param_dev(policy, names, z, tag, u):
    return float(np.abs(common.flat_params(policy, names) - z[tag + "_params"][u]).max())


def _run_variant(z, dev, tag, check_params, **attrs):
    """Six update() calls of one recorded variant; everything but the parameters is asserted
    here, the parameters by ``check_params(u, policy, names)``."""
    cfg, policy, v, buf = _setup(z, dev, tag, **attrs)
    kind, names = v["kind"], cfg["nets"][v["kind"]]
    seen = _record(policy)
    np.random.seed(cfg["seed"])
    prev = None
    for u in range(common.N_UPDATES):
        res = policy.update(v["bs"], buf)
        s = seen[u]
        q = f"{tag} update {u}"
        assert set(res) == set(common.loss_keys(kind))
        assert s["indices"].tolist() == z[tag + "_indices"][u].tolist(), q
        q_scale = float(np.abs(z[tag + "_q_obs"][u]).mean())
        want_ret, want_td = z[tag + "_returns"][u].reshape(-1), z[tag + "_td"][u]
        got_ret, got_td = s["returns"].cpu().numpy().reshape(-1), s["td"].cpu().numpy()
        with np.errstate(divide="ignore", invalid="ignore"):
            rel_ret, rel_td = np.abs(got_ret / want_ret - 1).max(), \
                np.abs(got_td / want_td - 1).max()
        print(f"{q}: " + " ".join(
            f"{k} {res[k]:.7g} ({float(z[tag + '_' + k.replace('/', '_')][u]):.7g})"
            for k in common.loss_keys(kind))
            + f" max rel returns {rel_ret:.3g} td {rel_td:.3g} max|dparam| "
            f"{_param_dev(policy, names, z, tag, u):.3g} mean|Q| {q_scale:.3g}")
        np.testing.assert_allclose(got_ret, want_ret, rtol=1e-5, err_msg=q)
        for k in common.loss_keys(kind)[1:]:
            np.testing.assert_allclose(res[k], float(z[tag + "_" + k.replace("/", "_")][u]),
                                       rtol=2e-5, err_msg=q)
        assert abs(res["loss/actor"] - float(z[tag + "_loss_actor"][u])) <= 2e-5 * q_scale, q
        if kind == "td3":
            assert policy._cnt == int(z[tag + "_cnt"][u]) == u + 1
            assert abs(policy._last - float(z[tag + "_last"][u])) <= 2e-5 * q_scale
            assert res["loss/actor"] == policy._last
            if u % v["freq"] != 0:  # no actor step: _last carried over, targets untouched
                assert res["loss/actor"] == prev["loss/actor"], q
        assert s["td"].is_cuda and not s["td"].requires_grad
        np.testing.assert_allclose(got_td, want_td, rtol=1e-4, err_msg=q)
        if v.get("per"):
            np.testing.assert_allclose(s["weight"].cpu().numpy(), z[tag + "_weight"][u],
                                       rtol=1e-6, err_msg=q)
            leaves = buf.weight[np.arange(buf.maxsize)]
            np.testing.assert_allclose(np.asarray(leaves), z[tag + "_leaves"][u], rtol=1e-4,
                                       err_msg=q)
        check_params(u, policy, names)
        prev = res
    if v.get("per"):
        np.testing.assert_allclose(buf._max_prio, float(z[tag + "_max_prio"]), rtol=1e-4)
        np.testing.assert_allclose(buf._min_prio, float(z[tag + "_min_prio"]), rtol=1e-4)
    return policy


def _adam_check(z, tag):
    def check(u, policy, names):
        np.testing.assert_allclose(common.flat_params(policy, names), z[tag + "_params"][u],
                                   rtol=1e-5, atol=1e-6, err_msg=f"{tag} update {u}")
    return check


@pytest.mark.parametrize("tag", common.ADAM_TAGS)
def test_update_matches_reference_adam(z, dev, tag):
    policy = _run_variant(z, dev, tag, _adam_check(z, tag))
    for name in policy._sync_order:
        st = policy._flats[name]
        assert st["fa"].adam_bound(getattr(policy, name + "_optim")), name
        assert policy._flat_pair(name) is not None, name
    assert policy._learn_graphs and not policy._graph_failed
    kinds = {k[-1] for k in policy._learn_graphs}
    freq = common.learn_cfg(z)["variants"][tag].get("freq", 1)
    # update 0 runs eagerly; of the replayed ones TD3 takes the critics-only graph too
    assert kinds == ({True} if freq == 1 else {True, False})


def test_update_matches_reference_rmsprop(z, dev):
    """Measured on an MI355X, max |parameter - recorded| after each update: see TORCH_DEV and
    the figures this test prints."""
    def check(u, policy, names):
        d = _param_dev(policy, names, z, "ddpg_rms", u)
        assert d <= 4 * TORCH_DEV["ddpg_rms"][u], (u, d)
    policy = _run_variant(z, dev, "ddpg_rms", check)
    assert policy._flats["critic"]["fa"].adam_bound(policy.critic_optim)
    assert set(policy.actor_optim.state[next(policy.actor.parameters())]) == \
        {"step", "square_avg"}


@pytest.mark.parametrize("tag", common.ADAM_TAGS)
def test_torch_formulation_matches_reference(z, dev, tag):
    """fused = False, the reference's op sequence on the GPU (the benchmark's comparison
    leg), meets the same bounds."""
    policy = _run_variant(z, dev, tag, _adam_check(z, tag), fused=False)
    assert not policy._flats and not policy._learn_graphs


def test_torch_formulation_rmsprop(z, dev):
    """The torch leg of the RMSprop variant: every other bound of the recording, and its
    parameter deviation (the figures behind TORCH_DEV, printed) inside the Adam bound."""
    devs = []

    def check(u, policy, names):
        devs.append(_param_dev(policy, names, z, "ddpg_rms", u))
        _adam_check(z, "ddpg_rms")(u, policy, names)
    _run_variant(z, dev, "ddpg_rms", check, fused=False)
    print("torch-leg RMSprop deviation per update:", " ".join(f"{d:.3g}" for d in devs))


# -- paths taken ------------------------------------------------------------------------------------
def test_flat_storage_is_bound_with_plain_adam(z, dev):
    cfg, policy, v, buf = _setup(z, dev, "td3")
    np.random.seed(3)
    policy.update(v["bs"], buf)
    for name in policy._sync_order:
        st = policy._flats[name]
        fa, optim = st["fa"], getattr(policy, name + "_optim")
        assert fa.adam_bound(optim)
        flat, old = fa.flat_param, st["old"]
        lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * 4
        for p in getattr(policy, name).parameters():
            assert lo <= p.data_ptr() < hi
            for key in ("exp_avg", "exp_avg_sq"):
                assert optim.state[p][key].shape == p.shape
                assert optim.state[p][key]._base is not None
        assert old is not None and old.shape == flat.shape and old.data_ptr() != lo
        storages = {p.untyped_storage().data_ptr()
                    for p in getattr(policy, name + "_old").parameters()}
        assert storages == {old.untyped_storage().data_ptr()}
        for p_old, p in zip(getattr(policy, name + "_old").parameters(), fa.params):
            assert p_old.data_ptr() - old.data_ptr() == p.data_ptr() - lo  # laid out alike
    # tau = 1: the soft update is a copy of every flat buffer
    policy.update(v["bs"], buf)
    policy.tau = 1.0
    policy.sync_weight()
    for name in policy._sync_order:
        st = policy._flats[name]
        assert torch.equal(st["old"], st["fa"].flat_param)
    assert not policy.actor_old.training and policy.train().critic1.training
    assert not policy.critic1_old.training


@pytest.mark.parametrize("tag", ("ddpg", "td3"))
def test_other_optimisers_keep_torch_step(z, dev, tag):
    cfg, policy, v, buf = _setup(z, dev, tag, optim="sgd")
    before = common.flat_params(policy, cfg["nets"][v["kind"]])
    np.random.seed(3)
    res = [policy.update(v["bs"], buf) for _ in range(3)]
    for name in policy._sync_order:
        assert not policy._flats[name]["fa"].adam_bound(getattr(policy, name + "_optim"))
        assert policy._flat_pair(name) is None
    assert not policy._learn_graphs
    losses = [r[k] for r in res for k in common.loss_keys(v["kind"])[1:]]
    assert all(np.isfinite(losses)) and len(set(losses)) == len(losses)
    after = common.flat_params(policy, cfg["nets"][v["kind"]])
    assert (before != after).mean() > 0.9  # online and target networks all moved


def test_mixed_optimisers_step_each_network_its_way(z, dev):
    """A plain Adam critic beside an SGD actor: the critic keeps its flat storage and the
    one-launch soft update, the actor torch's step; nothing is captured."""
    cfg = common.learn_cfg(z)
    nets = common.make_nets(z, cfg, "ddpg", dev)
    policy = DDPGPolicy(nets["actor"], common.make_optim("sgd", nets["actor"].parameters()),
                        nets["critic"], common.make_optim("adam", nets["critic"].parameters()),
                        tau=cfg["tau"], gamma=cfg["gamma"], exploration_noise=None,
                        action_scaling=False).to(dev)
    buf = _filled_buffer(z, cfg, dev)
    before = common.flat_params(policy, ["actor", "critic"])
    np.random.seed(3)
    for _ in range(2):
        res = policy.update(64, buf)
    assert policy._flat_pair("critic") is not None and policy._flat_pair("actor") is None
    assert not policy._learn_graphs and all(np.isfinite(list(res.values())))
    assert (before != common.flat_params(policy, ["actor", "critic"])).mean() > 0.9


def _updates(z, dev, tag, sizes, **attrs):
    cfg, policy, v, buf = _setup(z, dev, tag, **attrs)
    g = torch.Generator().manual_seed(9)  # any batch size: the same draws in both runs
    policy._smoothing_noise = lambda shape, device: \
        torch.randn(tuple(shape), generator=g).to(device)
    np.random.seed(cfg["seed"])
    out = []
    for bs in sizes:
        res = policy.update(bs, buf)
        out.append([res[k] for k in common.loss_keys(v["kind"])])
    return policy, out, common.flat_params(policy, cfg["nets"][v["kind"]])


@pytest.mark.parametrize("tag", ("ddpg", "ddpg_per", "ddpg_rms", "td3", "td3_per"))
def test_graph_replay_is_bitwise_eager(z, dev, tag):
    v = common.learn_cfg(z)["variants"][tag]
    sizes = [v["bs"]] * common.N_UPDATES
    pol_g, loss_g, par_g = _updates(z, dev, tag, sizes, graph_learn=True)
    pol_e, loss_e, par_e = _updates(z, dev, tag, sizes, graph_learn=False)
    # TD3's two step kinds are two graphs
    assert len(pol_g._learn_graphs) == (1 if v.get("freq", 1) == 1 else 2)
    assert not pol_e._learn_graphs
    assert loss_g == loss_e
    assert np.array_equal(par_g, par_e)


@pytest.mark.parametrize("tag", ("ddpg", "td3"))
def test_graph_replay_follows_batch_size(z, dev, tag):
    sizes = [64, 64, 32, 64, 32, 32]
    pol_g, loss_g, par_g = _updates(z, dev, tag, sizes, graph_learn=True)
    pol_e, loss_e, par_e = _updates(z, dev, tag, sizes, graph_learn=False)
    assert sorted({k[0] for k in pol_g._learn_graphs}) == [32, 64]
    assert loss_g == loss_e
    assert np.array_equal(par_g, par_e)


def test_actor_step_leaves_no_critic_gradient(z, dev):
    """The actor loss's backward runs through the critic; nothing of it may land in the
    critic's flat gradient bucket, which the next critic step reads."""
    cfg, policy, v, buf = _setup(z, dev, "ddpg", graph_learn=False)
    np.random.seed(3)
    policy.update(v["bs"], buf)
    fa, snap = policy._flats["critic"]["fa"], []
    clip_adam = fa.clip_adam
    fa.clip_adam = lambda *a, **k: (snap.append(fa.flat_grad.clone()), clip_adam(*a, **k))[1]
    policy.update(v["bs"], buf)
    assert len(snap) == 1 and float(snap[0].abs().sum()) > 0
    assert torch.equal(fa.flat_grad, snap[0])
    for p in policy.critic.parameters():
        assert p.grad is not None and p.grad.data_ptr() >= fa.flat_grad.data_ptr()


def test_capture_failure_warns_once_and_stays_eager(z, dev, monkeypatch):
    """A capture that raises RuntimeError (simulated on the host: the capture entry raises
    before torch.cuda.graph is entered, so no stream is ever capturing) warns once, latches
    _graph_failed and every update runs eagerly, still matching the recording."""
    tries = []

    def failing_capture(graph):
        tries.append(graph)
        raise RuntimeError("simulated capture failure")

    monkeypatch.setattr(ddpg_mod, "graph_capture", failing_capture)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        policy = _run_variant(z, dev, "td3", _adam_check(z, "td3"), graph_learn=True)
    msgs = [w for w in caught if "learn-graph capture failed" in str(w.message)]
    assert len(msgs) == 1 and len(tries) == 1
    assert policy._graph_failed and not policy._learn_graphs


def test_td3_smoothing_noise_default_draw(z, dev):
    cfg, policy, v, buf = _setup(z, dev, "td3")
    del policy._smoothing_noise  # the class's own: torch.randn on the device
    torch.manual_seed(4)
    a = policy._smoothing_noise((64, 3), dev)
    torch.manual_seed(4)
    assert torch.equal(a, torch.randn(size=(64, 3), device=dev))
    assert a.is_cuda and a.dtype == torch.float32
    np.random.seed(1)
    res = policy.update(v["bs"], buf)
    assert all(np.isfinite(list(res.values())))


# -- Collector --------------------------------------------------------------------------------------
def test_collect_with_exploration_noise_matches_reference(z, dev):
    """(c) of the recording: the actor's output layer is zero, so its action is exactly 0 on
    any GEMM and the stored action is the noise draw alone -- bitwise the reference's f64
    action rounded to f32.  Rewards, flags and episode statistics do not depend on the action:
    equal.  Observations carry f32(0.05 * remapped action): the reference remaps in f64 and
    rounds once, this package remaps the f32 action in f32 (three roundings at |a| <= 3, 3 *
    2^-23 * 0.05 ~ 2e-8) ahead of the final rounding of an |obs| < 4 (2.4e-7): atol 5e-7."""
    from tianshou_amd.data import Collector, VectorReplayBuffer
    from tianshou_amd.env import Box
    from tianshou_amd.env.synthetic import SyntheticVectorEnv
    from tianshou_amd.exploration import GaussianNoise
    from tianshou_amd.utils.net import Actor, Critic, Net
    c = json.loads(str(z["col_cfg"]))
    E, D, A = c["E"], c["D"], c["A"]
    env = SyntheticVectorEnv(E, (D,), A, ep_len=c["L"], seed=c["env_seed"], device=dev,
                             act_coef=c["act_coef"])
    space = Box(np.array(c["low"], np.float32), np.array(c["high"], np.float32), (A,))
    env.action_space = space
    actor = Actor(Net(D, hidden_sizes=(16, 16), device=dev), (A,), device=dev).to(dev)
    critic = Critic(Net(D, A, hidden_sizes=(16, 16), concat=True, device=dev), device=dev).to(dev)
    with torch.no_grad():
        for t in actor.last.parameters():
            t.zero_()
    policy = DDPGPolicy(actor, torch.optim.Adam(actor.parameters(), lr=1e-3), critic,
                        torch.optim.Adam(critic.parameters(), lr=1e-3),
                        exploration_noise=GaussianNoise(sigma=c["sigma"]), action_space=space,
                        action_scaling=True, action_bound_method="clip").to(dev)
    buf = VectorReplayBuffer(c["size"], E, device=dev)
    col = Collector(policy, env, buf, exploration_noise=True)
    assert col._noise_active()
    np.random.seed(c["seed"])
    res = col.collect(n_step=c["n_step"])
    common.assert_np_state(z, "col_")
    assert res["n/ep"] == int(z["col_n_ep"]) and res["n/st"] == int(z["col_n_st"])
    for k in ("lens", "idxs"):
        assert np.asarray(res[k]).tolist() == z["col_" + k].tolist(), k
    np.testing.assert_allclose(np.asarray(res["rews"]), z["col_rews"], rtol=1e-12)
    m = buf._meta
    want_act = z["col_buf_act"]
    assert want_act.dtype == np.float64 and (np.abs(want_act) > 1.0).any()
    got_act = m.act.cpu().numpy()
    assert got_act.dtype == np.float32 and got_act.shape == want_act.shape
    assert np.array_equal(got_act, want_act.astype(np.float32))
    for k in ("rew", "terminated", "truncated", "done"):
        got, want = getattr(m, k).cpu().numpy(), z["col_buf_" + k]
        assert got.shape == want.shape, k
        assert np.array_equal(got.astype(want.dtype), want), k
    for k in ("obs", "obs_next"):
        got, want = getattr(m, k).cpu().numpy(), z["col_buf_" + k]
        assert got.shape == want.shape and float(np.abs(want).max()) < 4.0, k
        print(k, "max |obs - recorded|", float(np.abs(got - want).max()))
        np.testing.assert_allclose(got, want, rtol=0, atol=5e-7, err_msg=k)
