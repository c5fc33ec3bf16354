"""SACPolicy on the device path (tianshou_amd/policy/sac.py, csrc/sac.hip) against f64
restatements and torch fp32 on the same device inputs (kernels), and against the reference run
recorded in tests/golden/sac.npz (tools/gen_goldens.py gen_sac; tests/test_sac_host.py pins
that file).

Kernel shapes are the lane, wave, workgroup and multi-partial edges, and an action width past
a wavefront, not workload sizes.  Tolerances: ``act`` within 2.0 ulp32 of f64 tanh of the f32
u; tsrl_sac_target bitwise; the actor / temperature losses rtol 1e-5 and their gradients rtol
1e-4 / atol 1e-6 * max|ref| (tsrl_q_mse_fwd_bwd's).  log_prob, g_mu and g_sigma: twice the
maximum error of the reference's f32 op sequence on the same device against the f64 value, and
at least 1 ulp32 of max|ref| -- both are one f32 evaluation of the same formula, the factor
absorbs another operation order.  Measured on an MI355X over every shape below, max |error|
against f64 (kernel / torch f32):
  log_prob  at most 1.49e-5 / 2.09e-5 (b 1000, A 65, max|ref| 47.6); the kernel's error was at
            most 1.42 x torch's in any shape (b 1, A 1: 3.50e-8 / 2.46e-8, under the 1 ulp floor)
  g_mu      at most 1.10e-6 / 6.22e-6; through log_prob the kernel stays under 8e-7 where torch
            shows 3e-6 to 6e-6 (its Gaussian terms cancel only up to rounding); through act
            alone both are 2e-8 to 4e-7, the kernel at most 2.7 x torch (b 1, A 17: 9.16e-8 /
            3.37e-8, under the 1 ulp floor of max|ref| 1.14)
  g_sigma   at most 1.80e-6 / 1.16e-5 (b 1000, A 65)
  act       at most 1.31 ulp32 (the library tanhf)
update() against the recording: sampled indices equal, returns rtol 1e-5 / atol 1e-6, critic
losses rtol 2e-5, outgoing weights rtol 1e-4, Adam parameters (online and target), log_alpha
and alpha rtol 1e-5 / atol 1e-6, priorities rtol 1e-4, actor and temperature losses by
sac_common.actor_loss_bound / alpha_loss_bound.  With RMSprop the parameter bound is 4 x what
the torch formulation of the same policy (``fused = False``) deviates from the same recording
on the same GPU (TORCH_DEV below), as in tests/test_gpu_ddpg.py."""
import json
import warnings

import numpy as np
import pytest
import torch

from tests import sac_common as common
from tests.test_gpu_ddpg import _bits, _filled_buffer, _record
from tianshou_amd import _C
from tianshou_amd.policy import SACPolicy
from tianshou_amd.policy import ddpg as ddpg_mod
from tianshou_amd.policy.sac import (EPS32, sac_actor_loss, sac_sample, sac_target_device)

pytestmark = pytest.mark.gpu

# max |parameter - recorded| (actor, critics and targets) of the torch formulation
# (fused = False) after each of the six updates of the "sac_rms" variant, measured on an MI355X
# against tests/golden/sac.npz (test_torch_formulation_rmsprop prints them).
TORCH_DEV = {
    "sac_rms": (6.71e-8, 7.45e-8, 7.45e-8, 7.45e-8, 7.45e-8, 7.45e-8),
}
# The fused path measured 5.96e-8 after the first four updates and 7.45e-8 after the last two
# in the same session, eager and replayed alike.  The Adam variants stay inside rtol 1e-5 / atol
# 1e-6, so the 4 x rule is not needed there.

BS = (1, 63, 64, 65, 257, 1000)
AS = (1, 3, 6, 17, 65)
LOG_SQRT_2PI = float(np.log(np.sqrt(2 * np.pi)))


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def z(golden_dir):
    return common.golden(golden_dir)


def _ulp32(x: torch.Tensor) -> torch.Tensor:
    """The spacing of f32 at |x| (f64 in, f64 out)."""
    a = x.abs().to(torch.float32)
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


# -- tsrl_sac_sample_fwd / _bwd ---------------------------------------------------------------------
def _sample_inputs(b, A, dev):
    """mu, sigma, eps with |u| <= 2.5."""
    g = torch.Generator().manual_seed(1000 * b + A)
    mu = (torch.rand(b, A, generator=g) * 2 - 1) * 0.9
    sigma = torch.exp((torch.rand(b, A, generator=g) * 2 - 1) * 0.7)
    eps = torch.randn(b, A, generator=g).clamp(-2.0, 2.0)
    eps = torch.maximum(torch.minimum(eps, (2.5 - mu) / sigma), (-2.5 - mu) / sigma) * 0.999
    g_act = torch.randn(b, A, generator=g)
    g_logp = torch.randn(b, generator=g)
    return [t.to(dev).contiguous() for t in (mu, sigma, eps, g_act, g_logp)]


def _reference(mu, sigma, eps, u=None):
    """sac.py:117-128 in the dtype of ``mu``: (act, log_prob [b]); ``u`` overrides the sample."""
    if u is None:
        u = mu if eps is None else mu + eps * sigma
    gauss = -((u - mu) ** 2) / (2 * sigma ** 2) - sigma.log() - LOG_SQRT_2PI
    act = torch.tanh(u)
    log_prob = gauss.sum(-1) - torch.log((1 - act.pow(2)) + EPS32).sum(-1)
    return act, log_prob


def _allowed(err_torch: float, ref: torch.Tensor) -> float:
    return max(2.0 * err_torch, float(_ulp32(ref.abs().max().double())))


@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("b", BS)
def test_sample_forward_matches_f64(dev, b, A):
    mu, sigma, eps, _, _ = _sample_inputs(b, A, dev)
    u32 = mu + eps * sigma  # torch's f32 rsample: two rounded operations
    assert float(u32.abs().max()) <= 2.5
    act, log_prob = sac_sample(mu, sigma, eps)
    assert act.shape == (b, A) and log_prob.shape == (b,)
    act64 = torch.tanh(u32.double())
    _, lp64 = _reference(mu.double(), sigma.double(), None, u=u32.double())
    _, lp32 = _reference(mu, sigma, eps)
    err_act = float(((act.double() - act64).abs() / _ulp32(act64)).max())
    err_k = float((log_prob.double() - lp64).abs().max())
    err_t = float((lp32.double() - lp64).abs().max())
    print(f"b {b} A {A}: act {err_act:.3f} ulp; log_prob max|err| kernel {err_k:.3g} torch "
          f"{err_t:.3g} of max|ref| {float(lp64.abs().max()):.3g}")
    assert err_act <= 2.0
    assert err_k <= _allowed(err_t, lp64)
    # a fixed order: the same bits every launch; a null eps is eps = 0
    act2, lp2 = sac_sample(mu, sigma, eps)
    assert torch.equal(_bits(act), _bits(act2)) and torch.equal(_bits(log_prob), _bits(lp2))
    act_n, lp_n = sac_sample(mu, sigma, None)
    act_0, lp_0 = sac_sample(mu, sigma, torch.zeros_like(eps))
    assert torch.equal(_bits(act_n), _bits(act_0)) and torch.equal(_bits(lp_n), _bits(lp_0))
    assert float(((act_n.double() - torch.tanh(mu.double())).abs()
                  / _ulp32(torch.tanh(mu.double()))).max()) <= 2.0


@pytest.mark.parametrize("A", (1, 3, 65))
def test_sample_saturated_rows(dev, A):
    """u = +-20: act is exactly +-1, every correction term exactly log(eps32), everything
    finite, and no gradient reaches mu through the log-probability."""
    b = 65
    mu, sigma, eps, g_act, g_logp = _sample_inputs(b, A, dev)
    mu[0], mu[1] = 20.0, -20.0
    eps[:2] = 0.0
    mu[2, 0], eps[2, 0] = 0.0, 20.0 / float(sigma[2, 0])  # saturated through the draw
    mu_k, sigma_k = mu.clone().requires_grad_(True), sigma.clone().requires_grad_(True)
    act, log_prob = sac_sample(mu_k, sigma_k, eps)
    assert torch.equal(act[0], torch.ones(A, device=dev))
    assert torch.equal(act[1], -torch.ones(A, device=dev)) and float(act[2, 0].detach()) == 1.0
    assert torch.isfinite(act).all() and torch.isfinite(log_prob).all()
    gauss = (-sigma[:2].double().log() - LOG_SQRT_2PI).sum(-1)
    corr = gauss - log_prob[:2].double()
    want = A * float(np.log(np.float64(EPS32)))
    print(f"A {A}: correction {corr.tolist()} want {want}")
    torch.testing.assert_close(corr, torch.full_like(corr, want), rtol=1e-6, atol=0)
    log_prob.backward(g_logp)
    assert torch.isfinite(mu_k.grad).all() and torch.isfinite(sigma_k.grad).all()
    assert float(mu_k.grad[:2].abs().max()) == 0.0 and float(mu_k.grad[2, 0]) == 0.0
    assert float(mu_k.grad[3:].abs().max()) > 0.0
    torch.testing.assert_close(sigma_k.grad[:2], (-g_logp[:2, None] / sigma[:2]), rtol=1e-6,
                               atol=0)


def _grads(fn, mu, sigma, eps, g_act, g_logp):
    m, s = mu.clone().requires_grad_(True), sigma.clone().requires_grad_(True)
    act, lp = fn(m, s, eps)
    seed = 0.0
    if g_act is not None:
        seed = seed + (act * g_act).sum()
    if g_logp is not None:
        seed = seed + (lp * g_logp).sum()
    seed.backward()
    return m.grad, s.grad


@pytest.mark.parametrize("which", ("act", "logp", "both"))
@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("b", (1, 65, 257, 1000))
def test_sample_backward_matches_f64_autograd(dev, b, A, which):
    mu, sigma, eps, g_act, g_logp = _sample_inputs(b, A, dev)
    ga = g_act if which in ("act", "both") else None
    gl = g_logp if which in ("logp", "both") else None
    d = lambda t: None if t is None else t.double()  # noqa: E731
    ref = _grads(_reference, d(mu), d(sigma), d(eps), d(ga), d(gl))
    tor = _grads(_reference, mu, sigma, eps, ga, gl)
    got = _grads(sac_sample, mu, sigma, eps, ga, gl)
    for name, r, t, k in zip(("g_mu", "g_sigma"), ref, tor, got):
        err_k = float((k.double() - r).abs().max())
        err_t = float((t.double() - r).abs().max())
        print(f"b {b} A {A} {which} {name}: max|err| kernel {err_k:.3g} torch {err_t:.3g} of "
              f"max|ref| {float(r.abs().max()):.3g}")
        assert err_k <= _allowed(err_t, r), name
    if which != "act":  # a null eps is eps = 0
        null = _grads(sac_sample, mu, sigma, None, ga, gl)
        zero = _grads(sac_sample, mu, sigma, torch.zeros_like(eps), ga, gl)
        assert torch.equal(null[0], zero[0]) and torch.equal(null[1], zero[1])


def test_sample_rejects_bad_arguments(dev):
    L, s = _C.lib(), _C.stream_ptr(dev)
    x = torch.ones(4, 3, device=dev)
    y, lp = torch.empty_like(x), torch.empty(4, device=dev)
    p = _C.ptr
    for args in ((p(x), p(x), None, 0, 3, p(y), p(lp)), (p(x), p(x), None, 4, 0, p(y), p(lp)),
                 (None, p(x), None, 4, 3, p(y), p(lp)), (p(x), p(x), None, 4, 3, p(y), None)):
        with pytest.raises(_C.TsrlError, match="tsrl_sac_sample_fwd"):
            _C.check(L.tsrl_sac_sample_fwd(*args, s), "tsrl_sac_sample_fwd")
    for args in ((p(x), None, p(x), None, None, 4, 3, p(y), p(y.clone())),
                 (p(x), None, p(x), p(x), None, 0, 3, p(y), p(y.clone())),
                 (None, None, p(x), p(x), None, 4, 3, p(y), p(y.clone()))):
        with pytest.raises(_C.TsrlError, match="tsrl_sac_sample_bwd"):
            _C.check(L.tsrl_sac_sample_bwd(*args, s), "tsrl_sac_sample_bwd")
    with pytest.raises(ValueError):
        sac_sample(x, x[:, :2], None)
    with pytest.raises(ValueError):
        sac_sample(x, x, x[:2])
    with pytest.raises(_C.TsrlError):
        sac_sample(x.cpu(), x.cpu(), None)


# -- tsrl_sac_target ----------------------------------------------------------------------------------
@pytest.mark.parametrize("b", BS)
def test_target_matches_torch_bitwise(dev, b):
    g = torch.Generator().manual_seed(b)
    q1, q2 = torch.randn(b, 1, generator=g), torch.randn(b, 1, generator=g)
    lp = torch.randn(b, 1, generator=g) * 3 - 2
    if b >= 3:
        q1[0], q2[1] = float("nan"), float("nan")
        q2[2] = q1[2]
    q1, q2, lp = q1.to(dev), q2.to(dev), lp.to(dev)
    for a in (0.2, 0.0, 1.7):
        alpha = torch.full((1,), a, device=dev)
        want = torch.min(q1, q2) - alpha * lp  # sac.py:141-144
        got = sac_target_device(q1, q2, lp, alpha)
        assert got.shape == want.shape
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan) and int(nan.sum()) == (2 if b >= 3 else 0)
        assert torch.equal(_bits(got)[~nan], _bits(want)[~nan]), a
        scalar = torch.min(q1, q2) - a * lp  # a Python float temperature: the same f32 value
        assert torch.equal(_bits(got)[~nan], _bits(scalar)[~nan]), a
    with pytest.raises(ValueError):
        sac_target_device(q1, q2, lp, torch.zeros(2, device=dev))
    with pytest.raises(_C.TsrlError, match="tsrl_sac_target"):
        _C.check(_C.lib().tsrl_sac_target(_C.ptr(q1), None, _C.ptr(lp), _C.ptr(alpha), b,
                                          _C.ptr(q1.clone()), _C.stream_ptr(dev)),
                 "tsrl_sac_target")


# -- tsrl_sac_actor_loss_fwd_bwd ------------------------------------------------------------------------
def _loss_inputs(b, dev, ties=False):
    g = torch.Generator().manual_seed(77 * b + ties)
    q1, q2 = torch.randn(b, generator=g) + 1.0, torch.randn(b, generator=g) + 1.0
    lp = torch.randn(b, generator=g) * 2 - 3
    if ties:
        q2[::3] = q1[::3]
    return q1.to(dev), q2.to(dev), lp.to(dev)


def _loss_reference(q1, q2, lp, alpha, log_alpha, te):
    """(actor loss, alpha loss, g_q1, g_q2, g_logp, g_log_alpha) in the dtype of ``q1``."""
    x = [t.clone().requires_grad_(True) for t in (q1, q2, lp)]
    actor = (alpha * x[2] - torch.min(x[0], x[1])).mean()
    actor.backward()
    la = log_alpha.clone().requires_grad_(True)
    alpha_loss = -(la * (lp + te)).mean()
    alpha_loss.backward()
    return actor.detach(), alpha_loss.detach(), x[0].grad, x[1].grad, x[2].grad, la.grad


@pytest.mark.parametrize("auto", (False, True))
@pytest.mark.parametrize("ties", (False, True))
@pytest.mark.parametrize("b", BS)
def test_actor_loss_matches_f64(dev, b, ties, auto):
    q1, q2, lp = _loss_inputs(b, dev, ties)
    alpha, log_alpha, te = torch.full((1,), 0.37, device=dev), \
        torch.full((1,), -0.8, device=dev), -3.0
    ref = _loss_reference(q1.double(), q2.double(), lp.double(), alpha.double(),
                          log_alpha.double(), te)
    tor = _loss_reference(q1, q2, lp, alpha, log_alpha, te)
    outs = []
    for _ in range(2):
        x = [t.clone().requires_grad_(True) for t in (q1, q2, lp)]
        handle, loss, g_la = sac_actor_loss(*x, alpha, log_alpha if auto else None, te)
        handle.backward()
        outs.append((loss.clone(), *(t.grad.clone() for t in x),
                     *((g_la.clone(),) if auto else ())))
    loss, grads = outs[0][0], outs[0][1:4]
    assert loss.shape == ((2,) if auto else (1,))
    print(f"b {b} ties {ties} auto {auto}: actor {loss[0].item():.7g} f64 {ref[0].item():.7g} "
          f"torch {tor[0].item():.7g}" + (f" alpha {loss[1].item():.7g} f64 "
                                          f"{ref[1].item():.7g}" if auto else ""))
    torch.testing.assert_close(loss[0].double(), ref[0], rtol=1e-5, atol=0)
    for name, k, r, t in zip(("g_q1", "g_q2", "g_logp"), grads, ref[2:5], tor[2:5]):
        torch.testing.assert_close(k.double(), r, rtol=1e-4, atol=1e-6 * float(r.abs().max()),
                                   msg=name)
        if name != "g_logp":  # the route of the min's gradient, ties included, is torch's
            assert torch.equal(k == 0, t == 0), name
            torch.testing.assert_close(k, t, rtol=1e-6, atol=0, msg=name)
    if ties:
        tie = (q1 == q2)
        assert int(tie.sum()) >= (b + 2) // 3
        assert torch.equal(grads[0][tie], grads[1][tie])
        torch.testing.assert_close(grads[0][tie].double(),
                                   torch.full_like(ref[2][tie], -0.5 / b), rtol=1e-6, atol=0)
    if auto:
        torch.testing.assert_close(loss[1].double(), ref[1], rtol=1e-5, atol=0)
        torch.testing.assert_close(outs[0][4].double(), ref[5], rtol=1e-5, atol=0)
    for a, c in zip(outs[0], outs[1]):  # a fixed summation order: the same bits every launch
        assert torch.equal(_bits(a), _bits(c))


def test_actor_loss_nan_rows_and_static_outputs(dev):
    q1, q2, lp = _loss_inputs(65, dev)
    q1[0], q2[1] = float("nan"), float("nan")
    alpha = torch.full((1,), 0.2, device=dev)
    tor = _loss_reference(q1, q2, lp, alpha, torch.zeros(1, device=dev), -3.0)
    x = [t.clone().requires_grad_(True) for t in (q1, q2, lp)]
    slot, g_la = torch.zeros(5, device=dev), torch.zeros(1, device=dev)
    handle, loss, g_out = sac_actor_loss(*x, alpha, torch.zeros(1, device=dev), -3.0, slot[2:4],
                                         g_la)
    handle.backward()
    assert g_out is g_la and loss.data_ptr() == slot[2:4].data_ptr()
    assert torch.isnan(slot[2]) and float(slot[:2].abs().sum()) == 0.0 and float(slot[4]) == 0.0
    assert float(slot[3]) == 0.0  # log_alpha = 0
    for k, t in zip((x[0].grad, x[1].grad), tor[2:4]):  # a NaN row: both critics, as torch
        torch.testing.assert_close(k, t, rtol=1e-6, atol=0)
    assert float(x[0].grad[0]) != 0.0 and float(x[1].grad[0]) != 0.0
    # a temperature moved on the device is read by the next launch
    q1, q2, lp = _loss_inputs(65, dev)
    before = sac_actor_loss(q1, q2, lp, alpha)[1].clone()
    alpha.fill_(0.9)
    after = sac_actor_loss(q1, q2, lp, alpha)[1]
    assert float(before) != float(after)
    torch.testing.assert_close(after[0].double(), (0.9 * lp - torch.min(q1, q2)).double().mean(),
                               rtol=1e-5, atol=0)


def test_actor_loss_rejects_bad_arguments(dev):
    L, s, p = _C.lib(), _C.stream_ptr(dev), _C.ptr
    b = 257
    q = torch.ones(b, device=dev)
    g1, g2, g3 = (torch.empty(b, device=dev) for _ in range(3))
    al, la, loss = torch.ones(1, device=dev), torch.zeros(1, device=dev), \
        torch.zeros(2, device=dev)
    parts = torch.zeros(4, dtype=torch.float64, device=dev)
    good = [p(q), p(q), p(q), p(al), p(la), -3.0, b, p(g1), p(g2), p(g3), p(parts), p(loss),
            p(la.clone())]
    for i, bad in ((6, 0), (0, None), (3, None), (10, None), (12, None), (11, None)):
        args = list(good)
        args[i] = bad
        with pytest.raises(_C.TsrlError, match="tsrl_sac_actor_loss_fwd_bwd"):
            _C.check(L.tsrl_sac_actor_loss_fwd_bwd(*args, s), "tsrl_sac_actor_loss_fwd_bwd")
    with pytest.raises(ValueError):
        sac_actor_loss(q, q[:5], q, al)
    with pytest.raises(ValueError):
        sac_actor_loss(q, q, q, torch.ones(2, device=dev))


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


def _run_variant(z, dev, tag, check_params, **attrs):
    """Six update() calls of one recorded variant with the recorded draws; everything but the
    networks' parameters is asserted here, those by ``check_params(u, policy)``."""
    cfg, policy, v, buf = _setup(z, dev, tag, **attrs)
    seen = _record(policy)
    np.random.seed(cfg["seed"])
    for u in range(common.N_UPDATES):
        res = policy.update(v["bs"], buf)
        s, q = seen[u], f"{tag} update {u}"
        assert set(res) == set(common.loss_keys(v["auto"]))
        assert s["indices"].tolist() == z[tag + "_indices"][u].tolist(), q
        want_ret, want_td = z[tag + "_returns"][u].reshape(-1), z[tag + "_td"][u]
        got_ret, got_td = s["returns"].cpu().numpy().reshape(-1), s["td"].cpu().numpy()
        print(f"{q}: " + " ".join(
            f"{k} {res[k]:.7g} ({float(z[tag + '_' + k.replace('/', '_')][u]):.7g})"
            for k in common.loss_keys(v["auto"]))
            + f" max|dreturns| {np.abs(got_ret - want_ret).max():.3g} max|dtd| "
            f"{np.abs(got_td - want_td).max():.3g} max|dparam| "
            f"{_param_dev(policy, z, tag, u):.3g} actor bound "
            f"{common.actor_loss_bound(z, tag, u):.3g}")
        np.testing.assert_allclose(got_ret, want_ret, rtol=1e-5, atol=1e-6, err_msg=q)
        for k in ("loss/critic1", "loss/critic2"):
            np.testing.assert_allclose(res[k], float(z[tag + "_" + k.replace("/", "_")][u]),
                                       rtol=2e-5, err_msg=q)
        assert abs(res["loss/actor"] - float(z[tag + "_loss_actor"][u])) <= \
            common.actor_loss_bound(z, tag, u), q
        if v["auto"]:
            assert abs(res["loss/alpha"] - float(z[tag + "_loss_alpha"][u])) <= \
                common.alpha_loss_bound(z, cfg, tag, u), q
            np.testing.assert_allclose(res["alpha"], float(z[tag + "_alpha"][u]), rtol=1e-5,
                                       atol=1e-6, err_msg=q)
            np.testing.assert_allclose(policy._log_alpha.detach().cpu().numpy(),
                                       z[tag + "_log_alpha"][u], rtol=1e-5, atol=1e-6, err_msg=q)
            assert float(policy._alpha) == res["alpha"]
        assert s["td"].is_cuda and not s["td"].requires_grad
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
    return policy


def _adam_check(z, tag):
    def check(u, policy):
        np.testing.assert_allclose(common.flat_params(policy), z[tag + "_params"][u],
                                   rtol=1e-5, atol=1e-6, err_msg=f"{tag} update {u}")
    return check


def _rms_check(z):
    def check(u, policy):
        d = _param_dev(policy, z, "sac_rms", u)
        assert d <= 4 * TORCH_DEV["sac_rms"][u], (u, d)
    return check


@pytest.mark.parametrize("graph", (True, False))
@pytest.mark.parametrize("tag", common.ADAM_TAGS)
def test_update_matches_reference_adam(z, dev, tag, graph):
    """graph True: update 0 eager, the others replayed; False: fused eager throughout."""
    policy = _run_variant(z, dev, tag, _adam_check(z, tag), graph_learn=graph)
    for name in policy._optim_order:
        assert policy._flats[name]["fa"].adam_bound(getattr(policy, name + "_optim")), name
        assert policy._flat_ready(name), name
    assert policy._flat_pair("critic1") is not None and "old" in policy._flats["actor"]
    assert policy._flats["actor"]["old"] is None and not hasattr(policy, "actor_old")
    if policy._is_auto_alpha:
        assert policy._alpha_fa.adam_bound(policy._alpha_optim)
    assert not policy._graph_failed and len(policy._learn_graphs) == (1 if graph else 0)


@pytest.mark.parametrize("graph", (True, False))
def test_update_matches_reference_rmsprop(z, dev, graph):
    """Measured on an MI355X, max |parameter - recorded| after each update: see TORCH_DEV and
    the figures this test prints."""
    policy = _run_variant(z, dev, "sac_rms", _rms_check(z), graph_learn=graph)
    assert policy._flats["actor"]["fa"].adam_bound(policy.actor_optim)
    assert policy._alpha_fa.adam_bound(policy._alpha_optim)
    assert set(policy._alpha_optim.state[policy._log_alpha]) == {"step", "square_avg"}
    assert len(policy._learn_graphs) == (1 if graph else 0)


@pytest.mark.parametrize("tag", common.ADAM_TAGS)
def test_torch_formulation_matches_reference(z, dev, tag):
    """fused = False, the reference's op sequence on the GPU (the benchmark's comparison
    leg), meets the same bounds."""
    policy = _run_variant(z, dev, tag, _adam_check(z, tag), fused=False)
    assert not policy._flats and not policy._learn_graphs and policy._alpha_fa is None


def test_torch_formulation_rmsprop(z, dev):
    """The torch leg of the RMSprop variant: every other bound of the recording, and its
    parameter deviation (the figures behind TORCH_DEV, printed) inside the Adam bound."""
    devs = []

    def check(u, policy):
        devs.append(_param_dev(policy, z, "sac_rms", u))
        _adam_check(z, "sac_rms")(u, policy)
    _run_variant(z, dev, "sac_rms", check, fused=False)
    print("torch-leg RMSprop deviation per update:", " ".join(f"{d:.3g}" for d in devs))


# -- paths taken ------------------------------------------------------------------------------------
def _updates(z, dev, tag, sizes, **attrs):
    cfg, policy, v, buf = _setup(z, dev, tag, feed=False, **attrs)
    g = torch.Generator().manual_seed(9)  # any batch size: the same draws in both runs
    policy._rsample_noise = lambda shape, device: \
        torch.randn(tuple(shape), generator=g).to(device)
    np.random.seed(cfg["seed"])
    out = []
    for bs in sizes:
        res = policy.update(bs, buf)
        out.append([res[k] for k in common.loss_keys(v["auto"])])
    extra = [] if not v["auto"] else policy._log_alpha.detach().cpu().numpy().tolist()
    return policy, out, np.concatenate([common.flat_params(policy), extra])


@pytest.mark.parametrize("tag", common.TAGS)
def test_graph_replay_is_bitwise_eager(z, dev, tag):
    sizes = [64, 64, 32, 64, 32, 32]
    pol_g, loss_g, par_g = _updates(z, dev, tag, sizes, graph_learn=True)
    pol_e, loss_e, par_e = _updates(z, dev, tag, sizes, graph_learn=False)
    assert sorted(k[0] for k in pol_g._learn_graphs) == [32, 64]
    assert not pol_e._learn_graphs
    assert loss_g == loss_e
    assert np.array_equal(par_g, par_e)


def test_graph_follows_deterministic_eval_and_moved_storage(z, dev):
    """In eval mode with deterministic_eval an update draws nothing: another graph key.  A
    rebuilt optimiser moves the flat storage and drops the captured graphs."""
    cfg, policy, v, buf = _setup(z, dev, "sac_auto", feed=False, graph_learn=True)
    calls = []
    policy._rsample_noise = lambda shape, device: (
        calls.append(tuple(shape)), torch.zeros(tuple(shape), device=device))[1]
    np.random.seed(3)
    for _ in range(3):
        policy.update(32, buf)
    assert calls == [(32, 3)] * 6 and len(policy._learn_graphs) == 1
    policy.train(False)
    for _ in range(2):
        res = policy.update(32, buf)
    assert len(calls) == 6 and len(policy._learn_graphs) == 2
    assert all(np.isfinite(list(res.values())))
    policy.train()
    policy.actor_optim = torch.optim.Adam(policy.actor.parameters(), lr=1e-3)
    policy.update(32, buf)
    policy.update(32, buf)
    assert len(policy._learn_graphs) == 1


def test_actor_step_leaves_no_critic_gradient(z, dev):
    """The actor loss's backward runs through both critics; nothing of it may land in their
    flat gradient buckets, which the next critic step reads."""
    cfg, policy, v, buf = _setup(z, dev, "sac_auto", feed=False, graph_learn=False)
    np.random.seed(3)
    policy.update(v["bs"], buf)
    snaps = {}
    for name in ("critic1", "critic2"):
        fa = policy._flats[name]["fa"]
        clip_adam = fa.clip_adam

        def snap(*a, _fa=fa, _clip=clip_adam, _name=name, **k):
            snaps.setdefault(_name, []).append(_fa.flat_grad.clone())
            return _clip(*a, **k)
        fa.clip_adam = snap
    policy.update(v["bs"], buf)
    for name in ("critic1", "critic2"):
        fa = policy._flats[name]["fa"]
        assert len(snaps[name]) == 1 and float(snaps[name][0].abs().sum()) > 0
        assert torch.equal(fa.flat_grad, snaps[name][0])


def test_flat_storage_is_bound_with_plain_adam(z, dev):
    cfg, policy, v, buf = _setup(z, dev, "sac_auto", feed=False)
    np.random.seed(3)
    policy.update(v["bs"], buf)
    for name in policy._optim_order:
        fa, optim = policy._flats[name]["fa"], getattr(policy, name + "_optim")
        assert fa.adam_bound(optim)
        lo, hi = fa.flat_param.data_ptr(), fa.flat_param.data_ptr() + fa.flat_param.numel() * 4
        assert all(lo <= p.data_ptr() < hi for p in getattr(policy, name).parameters())
    for name in policy._sync_order:
        st = policy._flats[name]
        storages = {p.untyped_storage().data_ptr()
                    for p in getattr(policy, name + "_old").parameters()}
        assert storages == {st["old"].untyped_storage().data_ptr()}
    fa = policy._alpha_fa
    assert fa.adam_bound(policy._alpha_optim) and fa.flat_param.numel() == 1
    assert policy._log_alpha.data_ptr() == fa.flat_param.data_ptr()
    assert policy._log_alpha.grad.data_ptr() == fa.flat_grad.data_ptr()
    policy.update(v["bs"], buf)
    policy.tau = 1.0
    policy.sync_weight()
    for name in policy._sync_order:
        st = policy._flats[name]
        assert torch.equal(st["old"], st["fa"].flat_param)
    assert not policy.critic1_old.training and policy.train().critic1.training


def test_other_optimisers_keep_torch_step(z, dev):
    cfg, policy, v, buf = _setup(z, dev, "sac_auto", feed=False, optim="sgd")
    before = common.flat_params(policy)
    np.random.seed(3)
    res = [policy.update(v["bs"], buf) for _ in range(3)]
    for name in policy._optim_order:
        assert not policy._flats[name]["fa"].adam_bound(getattr(policy, name + "_optim"))
        assert not policy._flat_ready(name)
    assert not policy._alpha_fa.adam_bound(policy._alpha_optim)
    assert not policy._learn_graphs
    vals = [r[k] for r in res for k in common.loss_keys(True)]
    assert all(np.isfinite(vals))
    assert len({r["alpha"] for r in res}) == 3 and float(policy._log_alpha.detach()) != 0.0
    assert (before != common.flat_params(policy)).mean() > 0.9


def test_mixed_optimisers_step_each_network_its_way(z, dev):
    """Plain Adam critics and actor beside an SGD temperature: the networks keep their flat
    storage and the one-launch soft update, log_alpha torch's step on the kernel's gradient;
    nothing is captured.  Then an SGD actor beside Adam critics and temperature."""
    cfg, policy, v, buf = _setup(z, dev, "sac_auto", feed=False, alpha_kind="sgd")
    np.random.seed(3)
    g_seen = []
    step = policy._alpha_optim.step
    policy._alpha_optim.step = lambda: (g_seen.append(policy._log_alpha.grad.clone()), step())[1]
    for _ in range(2):
        res = policy.update(64, buf)
    assert all(policy._flat_ready(name) for name in policy._optim_order)
    assert not policy._alpha_fa.adam_bound(policy._alpha_optim) and not policy._learn_graphs
    assert len(g_seen) == 2 and all(np.isfinite(list(res.values())))
    torch.testing.assert_close(policy._log_alpha.detach(),
                               -cfg["alpha_lr"] * (g_seen[0] + g_seen[1]), rtol=1e-6, atol=0)
    assert res["alpha"] == float(policy._log_alpha.detach().exp())

    cfg = common.learn_cfg(z)
    nets = common.make_nets(z, cfg, cfg["variants"]["sac_auto"], dev)
    opt = {n: common.make_optim("sgd" if n == "actor" else "adam", m.parameters())
           for n, m in nets.items()}
    log_alpha = torch.zeros(1, requires_grad=True, device=dev)
    policy = SACPolicy(nets["actor"], opt["actor"], nets["critic1"], opt["critic1"],
                       nets["critic2"], opt["critic2"], tau=cfg["tau"], gamma=cfg["gamma"],
                       alpha=(-3.0, log_alpha, torch.optim.Adam([log_alpha], lr=3e-3)),
                       action_scaling=False).to(dev)
    before = common.flat_params(policy)
    for _ in range(2):
        res = policy.update(64, buf)
    assert policy._flat_ready("critic1") and policy._flat_ready("critic2")
    assert not policy._flat_ready("actor") and policy._alpha_fa.adam_bound(policy._alpha_optim)
    assert not policy._learn_graphs and all(np.isfinite(list(res.values())))
    assert (before != common.flat_params(policy)).mean() > 0.9


def test_capture_failure_warns_once_and_stays_eager(z, dev, monkeypatch):
    tries = []

    def failing_capture(graph):
        tries.append(graph)
        raise RuntimeError("simulated capture failure")

    monkeypatch.setattr(ddpg_mod, "graph_capture", failing_capture)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        policy = _run_variant(z, dev, "sac_auto", _adam_check(z, "sac_auto"), graph_learn=True)
    msgs = [w for w in caught if "learn-graph capture failed" in str(w.message)]
    assert len(msgs) == 1 and len(tries) == 1
    assert policy._graph_failed and not policy._learn_graphs


# -- hook and forward ---------------------------------------------------------------------------------
def test_default_rsample_noise(z, dev):
    cfg, policy, v, buf = _setup(z, dev, "sac", feed=False)
    torch.manual_seed(4)
    a = policy._rsample_noise((4096, 3), dev)
    torch.manual_seed(4)
    assert torch.equal(a, torch.randn(size=(4096, 3), device=dev))
    assert a.is_cuda and a.dtype == torch.float32 and a.shape == (4096, 3)
    assert abs(float(a.mean())) < 0.05 and abs(float(a.var()) - 1.0) < 0.05
    np.random.seed(1)
    res = policy.update(v["bs"], buf)
    assert all(np.isfinite(list(res.values())))


def test_forward_modes_and_recorded_forwards(z, dev):
    from tianshou_amd.data import Batch
    cfg, policy, v, buf = _setup(z, dev, "sac", feed=False)
    obs = torch.as_tensor(z["fwd_obs"], device=dev)
    for mode in ("eval", "train"):
        policy.train(mode == "train")
        common.feed_draws(policy, [z["fwd_train_eps"]] if mode == "train" else [])
        with torch.no_grad():
            res = policy(Batch(obs=obs, info=Batch()))
        assert set(res.keys()) == {"logits", "act", "state", "dist", "log_prob"}
        assert res.act.is_cuda and res.log_prob.shape == (len(obs), 1)
        assert isinstance(res.dist, torch.distributions.Independent)
        mu = res.logits[0]
        np.testing.assert_allclose(mu.cpu().numpy(), z[f"fwd_{mode}_mu"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(res.act.cpu().numpy(), z[f"fwd_{mode}_act"], rtol=1e-5,
                                   atol=1e-6)
        # mu to 1e-6 moves each of the A = 3 terms of log_prob by up to |c| <= 2 times that
        np.testing.assert_allclose(res.log_prob.cpu().numpy(), z[f"fwd_{mode}_log_prob"],
                                   rtol=1e-5, atol=1e-5)
        if mode == "eval":  # deterministic_eval: tanh(mu)
            want = torch.tanh(mu.double())
            assert float(((res.act.double() - want).abs() / _ulp32(want)).max()) <= 2.0
    # gradients reach the actor through both outputs
    policy.train()
    common.feed_draws(policy, [z["fwd_train_eps"]])
    res = policy(Batch(obs=obs, info=Batch()))
    (res.act.sum() + res.log_prob.sum()).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all()
               for p in policy.actor.parameters())


# -- Collector --------------------------------------------------------------------------------------
def test_collect_matches_reference(z, dev):
    """(c) of the recording: the output layers of mu and sigma are zero, so mu = 0 and sigma =
    1 on any GEMM and the stored action is tanh(draw): within 2.0 ulp32 of f64 tanh.  Rewards,
    flags and episode statistics do not depend on the action: equal.  Observations carry
    f32(0.05 * remapped action), held to tests/test_gpu_ddpg.py's collect tolerance (atol
    5e-7 on |obs| < 4)."""
    from tianshou_amd.data import Collector, VectorReplayBuffer
    from tianshou_amd.env import Box
    from tianshou_amd.env.synthetic import SyntheticVectorEnv
    from tianshou_amd.utils.net import ActorProb, Critic, Net
    c = json.loads(str(z["col_cfg"]))
    E, D, A = c["E"], c["D"], c["A"]
    env = SyntheticVectorEnv(E, (D,), A, ep_len=c["L"], seed=c["env_seed"], device=dev,
                             act_coef=c["act_coef"])
    space = Box(np.array(c["low"], np.float32), np.array(c["high"], np.float32), (A,))
    env.action_space = space
    actor = ActorProb(Net(D, hidden_sizes=(16, 16), device=dev), (A,), device=dev,
                      unbounded=True, conditioned_sigma=True).to(dev)
    critics = [Critic(Net(D, A, hidden_sizes=(16, 16), concat=True, device=dev),
                      device=dev).to(dev) for _ in range(2)]
    with torch.no_grad():
        for head in (actor.mu, actor.sigma):
            for t in list(head.parameters())[-2:]:
                t.zero_()
    policy = SACPolicy(actor, torch.optim.Adam(actor.parameters(), lr=1e-3), critics[0],
                       torch.optim.Adam(critics[0].parameters(), lr=1e-3), critics[1],
                       torch.optim.Adam(critics[1].parameters(), lr=1e-3), action_space=space,
                       action_scaling=True, action_bound_method="clip").to(dev)
    policy.train()
    common.feed_draws(policy, list(z["col_eps"]))
    buf = VectorReplayBuffer(c["size"], E, device=dev)
    col = Collector(policy, env, buf)
    res = col.collect(n_step=c["n_step"])
    with pytest.raises(StopIteration):  # one draw per vector step, none left
        policy._rsample_noise((E, A), dev)
    assert res["n/ep"] == int(z["col_n_ep"]) and res["n/st"] == int(z["col_n_st"])
    for k in ("lens", "idxs"):
        assert np.asarray(res[k]).tolist() == z["col_" + k].tolist(), k
    np.testing.assert_allclose(np.asarray(res["rews"]), z["col_rews"], rtol=1e-12)
    m = buf._meta
    steps = c["n_step"] // E
    got_act = m.act.cpu().numpy()
    assert got_act.dtype == np.float32 and got_act.shape == z["col_buf_act"].shape
    want = np.tanh(z["col_eps"].astype(np.float64)).transpose(1, 0, 2)
    got = got_act.reshape(E, -1, A)[:, :steps].astype(np.float64)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    print("max |act - tanh(draw)| in ulp32:", float((np.abs(got - want) / ulp).max()))
    assert (np.abs(got - want) <= 2.0 * ulp).all()
    # the reference's f32 actions are within 2 ulp32 of tanh(draw) too (gen_sac asserts it):
    # 4 ulp32 of an |act| < 1 apart at the most
    np.testing.assert_allclose(got_act, z["col_buf_act"], rtol=0, atol=2.4e-7)
    for k in ("rew", "terminated", "truncated", "done"):
        g, w = getattr(m, k).cpu().numpy(), z["col_buf_" + k]
        assert g.shape == w.shape, k
        assert np.array_equal(g.astype(w.dtype), w), k
    for k in ("obs", "obs_next"):
        g, w = getattr(m, k).cpu().numpy(), z["col_buf_" + k]
        assert g.shape == w.shape and float(np.abs(w).max()) < 4.0, k
        print(k, "max |obs - recorded|", float(np.abs(g - w).max()))
        np.testing.assert_allclose(g, w, rtol=0, atol=5e-7, err_msg=k)
