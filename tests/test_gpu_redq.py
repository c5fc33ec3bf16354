"""REDQPolicy on the device path (tianshou_amd/policy/redq.py, csrc/redq.hip) against f64
restatements and torch fp32 on the same device inputs (kernels), and against the reference run
recorded in tests/golden/redq.npz (tools/gen_goldens.py gen_redq; tests/test_redq_host.py pins
that file).

Kernel shapes are the lane, wave, workgroup and multi-partial edges of the batch (b) and
ensemble sizes from one member to more than any lane count divides (E), not workload sizes.
Tolerances: tsrl_redq_target bitwise torch's op sequence in min mode and rtol 1e-6 in mean mode
(against the f64 mean rounded once, then torch's f32 subtraction: the summation order over at
most E terms is the kernel's only freedom); tsrl_redq_q_loss_fwd_bwd's loss rtol 1e-5, its
gradient and mean TD error rtol 1e-4 / atol 1e-6 * max|ref| (tsrl_q_mse_fwd_bwd's bounds in
tests/test_gpu_ddpg.py); tsrl_redq_actor_loss_fwd_bwd's losses rtol 1e-5 and its constant
gradients rtol 1e-6.
update() against the recording: sampled indices and subsets equal, returns rtol 1e-5 / atol
1e-6, critic loss rtol 2e-5, outgoing weights and priorities rtol 1e-4, log_alpha and alpha rtol
1e-5 / atol 1e-6, actor and temperature losses by redq_common.actor_loss_bound /
alpha_loss_bound.  Parameters (online and target): rtol 1e-5 / atol 1e-6 for the variants in
ABS_TAGS; for the others (RMSprop in any case) 4 x what the torch formulation of the same policy
(``fused = False``) deviates from the same recording on the same GPU (TORCH_DEV below), as in
tests/test_gpu_sac.py."""
import warnings

import numpy as np
import pytest
import torch

from tests import redq_common as common
from tests.test_gpu_ddpg import _bits, _filled_buffer, _record
from tianshou_amd import _C
from tianshou_amd.policy import ddpg as ddpg_mod
from tianshou_amd.policy.ddpg import q_mse_loss
from tianshou_amd.policy.redq import redq_actor_loss, redq_q_loss, redq_target_device

pytestmark = pytest.mark.gpu

# max |parameter - recorded| (actor, critics and targets) of the torch formulation
# (fused = False) after each of the six updates, measured on an MI355X against
# tests/golden/redq.npz (test_torch_formulation_deviation prints them for every variant).
TORCH_DEV = {
    "redq_rms": (1.49e-7, 1.49e-7, 1.49e-7, 1.49e-7, 1.49e-7, 1.49e-7),
}
# The fused path measured 1.19e-7 to 1.49e-7 there, eager and replayed alike.  The Adam
# variants, batched GEMMs and all, stay inside rtol 1e-5 / atol 1e-6 on the fused path (at most
# 8.94e-8; their torch legs 1.49e-8 to 2.98e-8), so the 4 x rule is not needed there: they are
# held to the absolute bound.
ABS_TAGS = common.ADAM_TAGS

BS = (1, 63, 64, 65, 257, 1000)
ES = (1, 2, 3, 10, 33)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def z(golden_dir):
    return common.golden(golden_dir)


def subset_sizes(E):
    return sorted({1, min(2, E), E})


# -- tsrl_redq_target ---------------------------------------------------------------------------------
def target_inputs(b, E):
    """qs [E, b, 1] and log_prob [b, 1] on the host; columns 1 and 2 (where there are that
    many) repeat one value across all members and across two of them."""
    g = torch.Generator().manual_seed(100 * b + E)
    qs = torch.randn(E, b, 1, generator=g) + 1.0
    lp = torch.randn(b, 1, generator=g) * 3 - 2
    if b >= 3:
        qs[:, 1] = qs[0, 1].clone()
        qs[E - 1, 2] = qs[0, 2].clone()
    return qs, lp


def draw_subset(E, M, seed=0):
    return np.random.RandomState(1000 * E + 10 * M + seed).choice(E, M, replace=False)


@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("b", BS)
def test_target_min_is_bitwise_torch(dev, b, E):
    qs, lp = (t.to(dev) for t in target_inputs(b, E))
    for M in subset_sizes(E):
        idx = draw_subset(E, M)
        for a in (0.2, 0.0, 1.7):
            alpha = torch.full((1,), a, device=dev)
            want, _ = torch.min(qs[idx, ...], dim=0)  # redq.py:150-155
            want -= alpha * lp
            got = redq_target_device(qs, idx, "min", lp, alpha)
            assert got.shape == want.shape == (b, 1)
            assert torch.equal(_bits(got), _bits(want)), (M, a)
            scalar, _ = torch.min(qs[idx, ...], dim=0)
            scalar -= a * lp  # a Python float temperature: the same f32 value
            assert torch.equal(_bits(got), _bits(scalar)), (M, a)


@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("b", BS)
def test_target_mean_matches_f64(dev, b, E):
    qs, lp = (t.to(dev) for t in target_inputs(b, E))
    for M in subset_sizes(E):
        idx = draw_subset(E, M, seed=1)
        mean64 = qs[idx, ...].double().mean(0)
        zero = torch.zeros(1, device=dev)
        got0 = redq_target_device(qs, idx, "mean", lp, zero)
        torch.testing.assert_close(got0.double(), mean64, rtol=1e-6, atol=0)
        alpha = torch.full((1,), 0.2, device=dev)
        want = mean64.float()
        want -= alpha * lp
        got = redq_target_device(qs, idx, "mean", lp, alpha)
        assert got.shape == (b, 1)
        torch.testing.assert_close(got, want, rtol=1e-6, atol=0)
        if b >= 3:  # one value in every member: its mean is that value
            col = qs[0, 1] - alpha * lp[1]
            torch.testing.assert_close(got[1], col, rtol=1e-6, atol=0)
        again = redq_target_device(qs, idx, "mean", lp, alpha)
        assert torch.equal(_bits(got), _bits(again))


@pytest.mark.parametrize("mode", ("min", "mean"))
def test_target_nan_rows_stay_in_their_column(dev, mode):
    E, b = 5, 65
    qs, lp = (t.to(dev) for t in target_inputs(b, E))
    idx = np.array([3, 0, 4])
    alpha = torch.full((1,), 0.2, device=dev)
    clean = redq_target_device(qs, idx, mode, lp, alpha)
    assert torch.isfinite(clean).all()
    qs[0, 7], qs[4, 64] = float("nan"), float("nan")  # members of the subset
    qs[1, 9], qs[2, 0] = float("nan"), float("nan")   # members outside it
    got = redq_target_device(qs, idx, mode, lp, alpha)
    nan = torch.isnan(got).flatten()
    assert nan.nonzero().flatten().tolist() == [7, 64]
    assert torch.equal(_bits(got)[~nan], _bits(clean)[~nan])
    lp[3] = float("nan")
    assert torch.isnan(redq_target_device(qs, idx, mode, lp, alpha)).flatten().nonzero() \
        .flatten().tolist() == [3, 7, 64]


def test_target_rejects_bad_subsets_and_arguments(dev):
    E, b = 5, 65
    qs, lp = (t.to(dev) for t in target_inputs(b, E))
    alpha = torch.full((1,), 0.2, device=dev)
    for bad in ([0, 5], [-1, 2], [1, 2, 1 << 20], [], [0, 1, 2, 3, 4, 0]):
        with pytest.raises(_C.TsrlError, match="tsrl_redq_target"):
            redq_target_device(qs, np.array(bad, dtype=np.int64), "min", lp, alpha)
    with pytest.raises(ValueError):
        redq_target_device(qs, np.array([0, 1]), "max", lp, alpha)
    with pytest.raises(ValueError):
        redq_target_device(qs, np.array([0, 1]), "min", lp[:5], alpha)
    with pytest.raises(ValueError):
        redq_target_device(qs, np.array([0, 1]), "min", lp, torch.zeros(2, device=dev))
    L, s, p = _C.lib(), _C.stream_ptr(dev), _C.ptr
    host = np.array([0, 1], dtype=np.int32)
    idx = torch.as_tensor(host, device=dev)
    q2, l1, out = qs.view(E, b).contiguous(), lp.view(b).contiguous(), \
        torch.empty(b, device=dev)
    good = [p(q2), E, b, p(idx), host.ctypes.data, 2, 0, p(l1), p(alpha), p(out)]
    _C.check(L.tsrl_redq_target(*good, s), "tsrl_redq_target")
    for i, bad in ((0, None), (1, 0), (2, 0), (3, None), (4, None), (5, 0), (5, 6), (6, 2),
                   (7, None), (8, None), (9, None)):
        args = list(good)
        args[i] = bad
        with pytest.raises(_C.TsrlError, match="tsrl_redq_target"):
            _C.check(L.tsrl_redq_target(*args, s), "tsrl_redq_target")


# -- tsrl_redq_q_loss_fwd_bwd ---------------------------------------------------------------------------
def q_loss_inputs(b, E):
    g = torch.Generator().manual_seed(31 * b + E)
    q = torch.randn(E, b, generator=g) + 1.0
    ret = torch.randn(b, generator=g) * 2
    w = torch.rand(b, generator=g) + 0.5
    return q, ret, w


def q_loss_reference(q, ret, w):
    """(loss, gq, td_mean) of redq.py:161-169 in f64."""
    q, ret = q.double(), ret.double()
    w = torch.ones_like(ret) if w is None else w.double()
    td = q - ret
    return (td.pow(2) * w).mean(), 2 * w * td / td.numel(), td.mean(0)


@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("b", BS)
def test_q_loss_matches_f64(dev, b, E, weighted):
    q, ret, w = (t.to(dev) for t in q_loss_inputs(b, E))
    w = w if weighted else None
    ref = q_loss_reference(q, ret, w)
    outs = []
    for _ in range(2):
        x = q.clone().requires_grad_(True)
        handle, loss, td = redq_q_loss(x, ret, w)
        handle.backward()
        outs.append((loss.clone(), x.grad.clone(), td.clone()))
    loss, gq, td = outs[0]
    assert loss.shape == (1,) and gq.shape == (E, b) and td.shape == (b,)
    print(f"b {b} E {E} weighted {weighted}: loss {loss.item():.7g} f64 {ref[0].item():.7g}")
    torch.testing.assert_close(loss[0].double(), ref[0], rtol=1e-5, atol=0)
    for name, k, r in (("gq", gq, ref[1]), ("td_mean", td, ref[2])):
        torch.testing.assert_close(k.double(), r, rtol=1e-4, atol=1e-6 * float(r.abs().max()),
                                   msg=name)
    for a, c in zip(*outs):  # a fixed summation order: the same bits every launch
        assert torch.equal(_bits(a), _bits(c))


@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("b", BS)
def test_q_loss_of_one_member_is_q_mse(dev, b, weighted):
    q, ret, w = (t.to(dev) for t in q_loss_inputs(b, 1))
    w = w if weighted else None
    x = q.clone().requires_grad_(True)
    handle, loss, td = redq_q_loss(x, ret, w)
    handle.backward()
    y = q[0].clone().requires_grad_(True)
    handle1, loss1, td1 = q_mse_loss([y], ret, w)
    handle1.backward()
    torch.testing.assert_close(loss, loss1, rtol=1e-6, atol=0)
    torch.testing.assert_close(x.grad[0], y.grad, rtol=1e-6, atol=0)
    torch.testing.assert_close(td, td1, rtol=1e-6, atol=0)


def test_q_loss_static_outputs_and_bad_arguments(dev):
    E, b = 3, 257
    q, ret, w = (t.to(dev) for t in q_loss_inputs(b, E))
    slot, td_out = torch.zeros(4, device=dev), torch.zeros(b, device=dev)
    handle, loss, td = redq_q_loss(q, ret, w, td_out, slot[:1])
    assert td is td_out and loss.data_ptr() == slot.data_ptr()
    assert float(slot[0]) > 0 and float(slot[1:].abs().sum()) == 0.0
    assert float(td_out.abs().sum()) > 0
    with pytest.raises(ValueError):
        redq_q_loss(q.flatten(), ret, w)
    with pytest.raises(ValueError):
        redq_q_loss(q, ret[:5], w)
    with pytest.raises(ValueError):
        redq_q_loss(q, ret, w, None, slot[:2])
    L, s, p = _C.lib(), _C.stream_ptr(dev), _C.ptr
    gq, parts = torch.empty_like(q), torch.zeros(2, dtype=torch.float64, device=dev)
    good = [p(q), p(ret), p(w), E, b, p(gq), p(td_out), p(parts), p(slot)]
    _C.check(L.tsrl_redq_q_loss_fwd_bwd(*good, s), "tsrl_redq_q_loss_fwd_bwd")
    for i, bad in ((0, None), (1, None), (3, 0), (4, 0), (5, None), (6, None), (7, None),
                   (8, None)):
        args = list(good)
        args[i] = bad
        with pytest.raises(_C.TsrlError, match="tsrl_redq_q_loss_fwd_bwd"):
            _C.check(L.tsrl_redq_q_loss_fwd_bwd(*args, s), "tsrl_redq_q_loss_fwd_bwd")


# -- tsrl_redq_actor_loss_fwd_bwd -----------------------------------------------------------------------
def actor_loss_inputs(b, E):
    g = torch.Generator().manual_seed(77 * b + E)
    q = torch.randn(E, b, generator=g) + 1.0
    lp = torch.randn(b, generator=g) * 2 - 3
    return q, lp


ALPHA, LOG_ALPHA, TARGET_ENTROPY = 0.37, -0.8, -3.0


def actor_loss_reference(q, lp):
    """(actor loss, alpha loss, gq, g_logp, g_log_alpha) of redq.py:176-189 in f64."""
    q, lp = q.double(), lp.double()
    E, b = q.shape
    m = (lp + TARGET_ENTROPY).mean()
    return ((ALPHA * lp - q.mean(0)).mean(), -LOG_ALPHA * m, torch.full_like(q, -1.0 / (E * b)),
            torch.full_like(lp, float(np.float32(ALPHA)) / b), -m)


@pytest.mark.parametrize("auto", (False, True))
@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("b", BS)
def test_actor_loss_matches_f64(dev, b, E, auto):
    q, lp = (t.to(dev) for t in actor_loss_inputs(b, E))
    alpha, log_alpha = torch.full((1,), ALPHA, device=dev), \
        torch.full((1,), LOG_ALPHA, device=dev)
    a32, la32 = float(alpha.double()), float(log_alpha.double())  # the f32 values the kernel reads
    ref = actor_loss_reference(q, lp)
    want_actor = (a32 * lp.double() - q.double().mean(0)).mean()
    want_alpha = -la32 * (lp.double() + TARGET_ENTROPY).mean()
    outs = []
    for _ in range(2):
        x, y = q.clone().requires_grad_(True), lp.clone().requires_grad_(True)
        handle, loss, g_la = redq_actor_loss(x, y, alpha, log_alpha if auto else None,
                                             TARGET_ENTROPY)
        handle.backward()
        outs.append((loss.clone(), x.grad.clone(), y.grad.clone(),
                     *((g_la.clone(),) if auto else ())))
    loss, gq, glp = outs[0][:3]
    assert loss.shape == ((2,) if auto else (1,)) and gq.shape == (E, b) and glp.shape == (b,)
    print(f"b {b} E {E} auto {auto}: actor {loss[0].item():.7g} f64 {want_actor.item():.7g}"
          + (f" alpha {loss[1].item():.7g} f64 {want_alpha.item():.7g}" if auto else ""))
    torch.testing.assert_close(loss[0].double(), want_actor, rtol=1e-5, atol=0)
    torch.testing.assert_close(gq.double(), ref[2], rtol=1e-6, atol=0)
    torch.testing.assert_close(glp.double(), ref[3], rtol=1e-6, atol=0)
    if auto:
        torch.testing.assert_close(loss[1].double(), want_alpha, rtol=1e-5, atol=0)
        torch.testing.assert_close(outs[0][3].double(), ref[4].reshape(1), rtol=1e-5, atol=0)
    for a, c in zip(*outs):
        assert torch.equal(_bits(a), _bits(c))


def test_actor_loss_static_outputs_and_moved_temperature(dev):
    q, lp = (t.to(dev) for t in actor_loss_inputs(65, 3))
    alpha = torch.full((1,), 0.2, device=dev)
    x, y = q.clone().requires_grad_(True), lp.clone().requires_grad_(True)
    slot, g_la = torch.zeros(4, device=dev), torch.zeros(1, device=dev)
    handle, loss, g_out = redq_actor_loss(x, y, alpha, torch.zeros(1, device=dev), -3.0,
                                          slot[1:3], g_la)
    handle.backward()
    assert g_out is g_la and loss.data_ptr() == slot[1:3].data_ptr()
    assert float(slot[0]) == 0.0 and float(slot[3]) == 0.0 and float(slot[1]) != 0.0
    assert float(slot[2]) == 0.0  # log_alpha = 0
    torch.testing.assert_close(g_la.double(), -(lp.double() - 3.0).mean().reshape(1),
                               rtol=1e-5, atol=0)
    # fixed temperature: the second slot and the gradient output stay untouched
    slot.zero_()
    redq_actor_loss(q, lp, alpha, loss_out=slot[1:2])
    assert float(slot[1]) != 0.0 and float(slot[2]) == 0.0
    # a temperature moved on the device is read by the next launch
    before = redq_actor_loss(q, lp, alpha)[1].clone()
    alpha.fill_(0.9)
    after = redq_actor_loss(q, lp, alpha)[1]
    assert float(before) != float(after)
    torch.testing.assert_close(after[0].double(),
                               (float(alpha.double()) * lp.double()
                                - q.double().mean(0)).mean(), rtol=1e-5, atol=0)


def test_actor_loss_rejects_bad_arguments(dev):
    L, s, p = _C.lib(), _C.stream_ptr(dev), _C.ptr
    E, b = 3, 257
    q, lp = torch.ones(E, b, device=dev), torch.ones(b, device=dev)
    gq, glp = torch.empty_like(q), torch.empty_like(lp)
    al, la, loss = torch.ones(1, device=dev), torch.zeros(1, device=dev), \
        torch.zeros(2, device=dev)
    parts = torch.zeros(4, dtype=torch.float64, device=dev)
    good = [p(q), p(lp), p(al), p(la), -3.0, E, b, p(gq), p(glp), p(parts), p(loss),
            p(la.clone())]
    _C.check(L.tsrl_redq_actor_loss_fwd_bwd(*good, s), "tsrl_redq_actor_loss_fwd_bwd")
    for i, bad in ((0, None), (1, None), (2, None), (5, 0), (6, 0), (7, None), (8, None),
                   (9, None), (10, None), (11, None)):
        args = list(good)
        args[i] = bad
        with pytest.raises(_C.TsrlError, match="tsrl_redq_actor_loss_fwd_bwd"):
            _C.check(L.tsrl_redq_actor_loss_fwd_bwd(*args, s), "tsrl_redq_actor_loss_fwd_bwd")
    with pytest.raises(ValueError):
        redq_actor_loss(q, lp[:5], al)
    with pytest.raises(ValueError):
        redq_actor_loss(q, lp, torch.ones(2, device=dev))
    with pytest.raises(ValueError):
        redq_actor_loss(q.flatten(), lp, al)


# -- update() against the recording -----------------------------------------------------------------
def _setup(z, dev, tag, feed=True, **attrs):
    cfg = common.learn_cfg(z)
    policy, v = common.make_policy(z, cfg, tag, dev, **attrs)
    policy.train()
    if feed:
        common.feed_draws(policy, common.update_draws(z, tag))
    return cfg, policy, v, _filled_buffer(z, cfg, dev, per=bool(v.get("per")))


def _param_dev(policy, z, tag, u):
    return float(np.abs(common.flat_params(policy) - z[tag + "_params"][u]).max())


def _spy_subsets(monkeypatch):
    subsets, choice = [], np.random.choice

    def spy(*a, **kw):
        res = choice(*a, **kw)
        if kw.get("replace") is False:
            subsets.append(np.array(res, copy=True))
        return res

    monkeypatch.setattr(np.random, "choice", spy)
    return subsets


def _run_variant(z, dev, tag, check_params, monkeypatch, **attrs):
    """Six update() calls of one recorded variant with the recorded draws; everything but the
    networks' parameters is asserted here, those by ``check_params(u, policy)``."""
    cfg, policy, v, buf = _setup(z, dev, tag, **attrs)
    seen, subsets = _record(policy), _spy_subsets(monkeypatch)
    np.random.seed(v["seed"])
    for u in range(common.N_UPDATES):
        res = policy.update(v["bs"], buf)
        s, q = seen[u], f"{tag} update {u}"
        did = common.did_actor(z, tag, u)
        keys = common.loss_keys(v["auto"], did)
        assert set(res) == set(keys), q
        assert policy.critic_gradient_step == u + 1
        assert s["indices"].tolist() == z[tag + "_indices"][u].tolist(), q
        assert len(subsets) == u + 1 and subsets[u].tolist() == z[tag + "_subset"][u].tolist(), q
        want_ret, want_td = z[tag + "_returns"][u].reshape(-1), z[tag + "_td"][u]
        got_ret, got_td = s["returns"].cpu().numpy().reshape(-1), s["td"].cpu().numpy()
        print(f"{q}: " + " ".join(
            f"{k} {res[k]:.7g} ({float(z[tag + '_' + k.replace('/', '_')][u]):.7g})"
            for k in keys)
            + f" max|dreturns| {np.abs(got_ret - want_ret).max():.3g} max|dtd| "
            f"{np.abs(got_td - want_td).max():.3g} max rel dtd "
            f"{np.abs(got_td / want_td - 1).max():.3g} max|dparam| "
            f"{_param_dev(policy, z, tag, u):.3g}"
            + (f" actor bound {common.actor_loss_bound(z, tag, u):.3g}" if did else ""))
        np.testing.assert_allclose(got_ret, want_ret, rtol=1e-5, atol=1e-6, err_msg=q)
        np.testing.assert_allclose(res["loss/critics"], float(z[tag + "_loss_critics"][u]),
                                   rtol=2e-5, err_msg=q)
        if did:
            assert isinstance(res["loss/actor"], float)
            assert abs(res["loss/actor"] - float(z[tag + "_loss_actor"][u])) <= \
                common.actor_loss_bound(z, tag, u), q
        if did and v["auto"]:
            assert abs(res["loss/alpha"] - float(z[tag + "_loss_alpha"][u])) <= \
                common.alpha_loss_bound(z, cfg, tag, u), q
            np.testing.assert_allclose(res["alpha"], float(z[tag + "_alpha"][u]), rtol=1e-5,
                                       atol=1e-6, err_msg=q)
            assert float(policy._alpha) == res["alpha"]
        if v["auto"]:
            np.testing.assert_allclose(policy._log_alpha.detach().cpu().numpy(),
                                       z[tag + "_log_alpha"][u], rtol=1e-5, atol=1e-6, err_msg=q)
        assert s["td"].is_cuda and not s["td"].requires_grad and s["td"].shape == (v["bs"],)
        np.testing.assert_allclose(got_td, want_td, rtol=1e-4, err_msg=q)
        if v.get("per"):
            np.testing.assert_allclose(s["weight"].cpu().numpy(), z[tag + "_weight"][u],
                                       rtol=1e-6, err_msg=q)
            leaves = buf.weight[np.arange(buf.maxsize)]
            np.testing.assert_allclose(np.asarray(leaves), z[tag + "_leaves"][u], rtol=1e-4,
                                       err_msg=q)
        check_params(u, policy)
    if v.get("per"):
        np.testing.assert_allclose(buf._max_prio, float(z[tag + "_max_prio"]), rtol=1e-4)
        np.testing.assert_allclose(buf._min_prio, float(z[tag + "_min_prio"]), rtol=1e-4)
    with pytest.raises(StopIteration):  # one draw per update and one more per actor step
        policy._rsample_noise((1, 1), dev)
    return policy


def _abs_check(z, tag):
    def check(u, policy):
        np.testing.assert_allclose(common.flat_params(policy), z[tag + "_params"][u],
                                   rtol=1e-5, atol=1e-6, err_msg=f"{tag} update {u}")
    return check


def _param_check(z, tag):
    if tag in ABS_TAGS:
        return _abs_check(z, tag)

    def check(u, policy):
        d = _param_dev(policy, z, tag, u)
        assert d <= 4 * TORCH_DEV[tag][u], (tag, u, d)
    return check


@pytest.mark.parametrize("graph", (True, False))
@pytest.mark.parametrize("tag", common.TAGS)
def test_update_matches_reference(z, dev, tag, graph, monkeypatch):
    """graph True: update 0 eager, the others replayed from the two graphs; False: fused eager
    throughout."""
    policy = _run_variant(z, dev, tag, _param_check(z, tag), monkeypatch, graph_learn=graph)
    for name in policy._optim_order:
        assert policy._flats[name]["fa"].adam_bound(getattr(policy, name + "_optim")), name
        assert policy._flat_ready(name), name
    assert policy._flat_pair("critics") is not None
    assert policy._flats["actor"]["old"] is None and not hasattr(policy, "actor_old")
    if policy._is_auto_alpha:
        assert policy._alpha_fa.adam_bound(policy._alpha_optim)
    kinds = {common.did_actor(z, tag, u) for u in range(1, common.N_UPDATES)}
    assert not policy._graph_failed
    assert len(policy._learn_graphs) == (len(kinds) if graph else 0)


@pytest.mark.parametrize("tag", common.TAGS)
def test_torch_formulation_deviation(z, dev, tag, monkeypatch):
    """fused = False, the reference's op sequence on the GPU (the benchmark's comparison leg):
    every other bound of the recording, and its parameter deviation -- the figures behind
    TORCH_DEV, printed -- inside rtol 1e-5 / atol 1e-6."""
    devs = []

    def check(u, policy):
        devs.append(_param_dev(policy, z, tag, u))
        _abs_check(z, tag)(u, policy)
    policy = _run_variant(z, dev, tag, check, monkeypatch, fused=False)
    print(f"torch-leg deviation per update, {tag}:", " ".join(f"{d:.3g}" for d in devs))
    assert not policy._flats and not policy._learn_graphs and policy._alpha_fa is None


# -- paths taken ------------------------------------------------------------------------------------
def _updates(z, dev, tag, sizes, **attrs):
    cfg, policy, v, buf = _setup(z, dev, tag, feed=False, **attrs)
    g = torch.Generator().manual_seed(9)  # any batch size: the same draws in both runs
    policy._rsample_noise = lambda shape, device: \
        torch.randn(tuple(shape), generator=g).to(device)
    np.random.seed(v["seed"])
    out = [sorted(policy.update(bs, buf).items()) for bs in sizes]
    extra = [] if not v["auto"] else policy._log_alpha.detach().cpu().numpy().tolist()
    return policy, out, np.concatenate([common.flat_params(policy), extra])


@pytest.mark.parametrize("tag", common.TAGS)
def test_graph_replay_is_bitwise_eager(z, dev, tag):
    sizes = [64, 64, 32, 64, 32, 32, 64, 32]
    pol_g, loss_g, par_g = _updates(z, dev, tag, sizes, graph_learn=True)
    pol_e, loss_e, par_e = _updates(z, dev, tag, sizes, graph_learn=False)
    assert {k[0] for k in pol_g._learn_graphs} == {32, 64}
    assert not pol_e._learn_graphs
    assert loss_g == loss_e
    assert np.array_equal(par_g, par_e)


def test_two_graphs_and_no_draw_on_critic_only_updates(z, dev):
    cfg, policy, v, buf = _setup(z, dev, "redq_auto", feed=False, graph_learn=True)
    assert v["delay"] == 3
    calls = []
    policy._rsample_noise = lambda shape, device: (
        calls.append(tuple(shape)), torch.zeros(tuple(shape), device=device))[1]
    np.random.seed(3)
    per_update = []
    for u in range(7):
        n0 = len(calls)
        res = policy.update(32, buf)
        per_update.append(len(calls) - n0)
        assert ("loss/actor" in res) == ((u + 1) % 3 == 0)
    # process_fn draws once; learn once more on the two actor updates and never otherwise
    assert per_update == [1, 1, 2, 1, 1, 2, 1] and set(calls) == {(32, 3)}
    assert len(policy._learn_graphs) == 2
    assert sorted(k[-1] for k in policy._learn_graphs) == [False, True]
    for key, st in policy._learn_graphs.items():  # obs, act, returns, weight (, the draw)
        assert len(st["static"]) == (5 if key[-1] else 4)
    # in eval mode with deterministic_eval nothing is drawn anywhere: a third graph
    policy.train(False)
    for _ in range(2):  # a critic-only update (the graph it had) and an actor update
        res = policy.update(32, buf)
    assert len(calls) == 9 and len(policy._learn_graphs) == 3
    assert "loss/actor" in res and all(np.isfinite(list(res.values())))


def test_actor_step_leaves_no_critic_gradient(z, dev):
    """The actor loss's backward runs through the ensemble; nothing of it may land in the
    critics' flat gradient bucket."""
    cfg, policy, v, buf = _setup(z, dev, "redq_full", feed=False, graph_learn=False)
    assert v["delay"] == 1
    np.random.seed(3)
    policy.update(v["bs"], buf)
    fa = policy._flats["critics"]["fa"]
    clip_adam, snaps = fa.clip_adam, []

    def snap(*a, **k):
        snaps.append(fa.flat_grad.clone())
        return clip_adam(*a, **k)
    fa.clip_adam = snap
    res = policy.update(v["bs"], buf)
    assert "loss/actor" in res
    assert len(snaps) == 1 and float(snaps[0].abs().sum()) > 0
    assert torch.equal(fa.flat_grad, snaps[0])


def test_flat_storage_is_bound_with_plain_adam(z, dev):
    cfg, policy, v, buf = _setup(z, dev, "redq_full", feed=False)
    np.random.seed(3)
    policy.update(v["bs"], buf)
    for name in policy._optim_order:
        fa, optim = policy._flats[name]["fa"], getattr(policy, name + "_optim")
        assert fa.adam_bound(optim)
        lo, hi = fa.flat_param.data_ptr(), fa.flat_param.data_ptr() + fa.flat_param.numel() * 4
        assert all(lo <= p.data_ptr() < hi for p in getattr(policy, name).parameters())
    st = policy._flats["critics"]
    storages = {p.untyped_storage().data_ptr() for p in policy.critics_old.parameters()}
    assert storages == {st["old"].untyped_storage().data_ptr()}
    fa = policy._alpha_fa
    assert fa.adam_bound(policy._alpha_optim) and fa.flat_param.numel() == 1
    assert policy._log_alpha.data_ptr() == fa.flat_param.data_ptr()
    assert policy._log_alpha.grad.data_ptr() == fa.flat_grad.data_ptr()
    policy.update(v["bs"], buf)
    policy.tau = 1.0
    policy.sync_weight()
    assert torch.equal(st["old"], st["fa"].flat_param)
    assert not policy.critics_old.training and policy.train().critics.training


def test_other_optimisers_keep_torch_step(z, dev):
    cfg, policy, v, buf = _setup(z, dev, "redq_full", feed=False, optim="sgd")
    before = common.flat_params(policy)
    np.random.seed(3)
    res = [policy.update(v["bs"], buf) for _ in range(3)]
    for name in policy._optim_order:
        assert not policy._flats[name]["fa"].adam_bound(getattr(policy, name + "_optim"))
        assert not policy._flat_ready(name)
    assert not policy._alpha_fa.adam_bound(policy._alpha_optim)
    assert not policy._learn_graphs
    vals = [r[k] for r in res for k in common.loss_keys(True, True)]
    assert all(np.isfinite(vals))
    assert len({r["alpha"] for r in res}) == 3 and float(policy._log_alpha.detach()) != 0.0
    assert (before != common.flat_params(policy)).mean() > 0.9


def test_capture_failure_warns_once_and_stays_eager(z, dev, monkeypatch):
    tries = []

    def failing_capture(graph):
        tries.append(graph)
        raise RuntimeError("simulated capture failure")

    monkeypatch.setattr(ddpg_mod, "graph_capture", failing_capture)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        policy = _run_variant(z, dev, "redq_auto", _param_check(z, "redq_auto"), monkeypatch,
                              graph_learn=True)
    msgs = [w for w in caught if "learn-graph capture failed" in str(w.message)]
    assert len(msgs) == 1 and len(tries) == 1
    assert policy._graph_failed and not policy._learn_graphs


# -- forward ------------------------------------------------------------------------------------------
def test_forward_modes_and_recorded_forwards(z, dev):
    from tianshou_amd.data import Batch
    cfg, policy, v, buf = _setup(z, dev, "redq", feed=False)
    obs = torch.as_tensor(z["fwd_obs"], device=dev)
    for mode in ("eval", "train"):
        policy.train(mode == "train")
        common.feed_draws(policy, [z["fwd_train_eps"]] if mode == "train" else [])
        with torch.no_grad():
            res = policy(Batch(obs=obs, info=Batch()))  # eval: a draw would raise StopIteration
        assert set(res.keys()) == {"logits", "act", "state", "dist", "log_prob"}
        assert res.act.is_cuda and res.log_prob.shape == (len(obs), 1)
        assert isinstance(res.dist, torch.distributions.Independent)
        np.testing.assert_allclose(res.logits[0].cpu().numpy(), z[f"fwd_{mode}_mu"], rtol=1e-5,
                                   atol=1e-6)
        np.testing.assert_allclose(res.act.cpu().numpy(), z[f"fwd_{mode}_act"], rtol=1e-5,
                                   atol=1e-6)
        # mu to 1e-6 moves each of the A = 3 terms of log_prob by up to |c| <= 2 times that
        np.testing.assert_allclose(res.log_prob.cpu().numpy(), z[f"fwd_{mode}_log_prob"],
                                   rtol=1e-5, atol=1e-5)
    with torch.no_grad():
        q = policy.critics(obs, torch.as_tensor(z["fwd_act_in"], device=dev))
    assert q.shape == (cfg["ensemble"], len(obs), 1)
    np.testing.assert_allclose(q.cpu().numpy(), z["fwd_q"], rtol=1e-5, atol=1e-6)
